"""pbr_denoise_temporal / pbr_temporal_reset (include/pbr_hip.h, csrc/pt_temporal.hpp): the guided filter with a per-pixel
history that is re-projected through the previous call's camera.

The integration (steps 1 to 4 of the header's definition) is a fixed binary32 algorithm: `integrated` and `history` are
compared with `same_values` (tolerance 0) against tests/temporal_ref.py, fed with the device's own accumulation, variance and
feature buffers and with the previous call's `integrated` and `history`.  The filter stage goes through expf and is compared as
test_gpu_guided_denoise.py compares it: rtol 2e-5, atol 1e-6 + 4 D, D = the largest colour difference between the restatement
with float32 exp and with float64 exp on the same input — measured on the reference side, never on the device.

Scene as in test_gpu_guided_denoise.py: HostScene.generate( "cornell", 1, 0 ), render.max_depth 4; 96 x 64, 8 frames per call
unless noted.  Cameras come from pbrh_camera_lookat; every call is preceded by reset_accum and a uniform adaptive round with a
seed range of its own."""
import ctypes
import types

import numpy as np
import pytest

import guided_denoise_ref
import temporal_ref as ref
from conftest import same_values, describe_mismatch

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 96, 64
FRAMES = 8


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def cornell(pbr, dev, brdf=1, w=W, h=H, **more):
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 4, "render.brdf": brdf})
    sc = pbr.HostScene.generate("cornell", 1, 0)
    cfg, px = sc.config(w, h), pbr.pixel_dimension(w, h)
    for key, value in more.items():
        setattr(cfg, key, value)
    dev.upload_scene(sc.desc)
    dev.configure(cfg)
    return sc, cfg, px


def view(pbr, sc, right=0.0, up=0.0, forward=0.0, turn=0.0):
    """A lookat camera: the scene's own eye moved by (right, up, forward) along its basis, looking at a point one unit ahead
    that is moved along with it and then `turn` units to the right (a small rotation about the up axis)."""
    base = sc.camera()
    eye, u, v, w = (np.array([getattr(base, k).x, getattr(base, k).y, getattr(base, k).z], np.float64) for k in ("eye", "u", "v", "w"))
    e = (eye + right * u + up * v + forward * w).astype(F)
    c = (e + w + turn * u).astype(F)
    cam = pbr.Camera()
    pbr.host.pbrh_camera_lookat(e.ctypes.data_as(pbr._fp), c.ctypes.data_as(pbr._fp), cam)
    return cam


def render(pbr, dev, px, cam, seed0, frames=FRAMES):
    """reset_accum + one adaptive round that every tile renders, with the seeds seed0 .. seed0 + frames - 1."""
    dev.reset_accum()
    dev.render_adaptive(0, pbr.frame_seeds(seed0, frames), px, cam, frames, frames, frames, 0.0)
    assert (dev.tile_stats()[0] == frames).all()


def step(pbr, dev, px, cam, seed0, temporal=None, filt=None, frames=FRAMES):
    """One displayed frame: render, then pbr_denoise_temporal with every optional output; the inputs of the restatement are
    read from the device before the call."""
    render(pbr, dev, px, cam, seed0, frames)
    s = types.SimpleNamespace(cam=cam, px=px)
    s.image, s.var = dev.read_output(), dev.read_variance()
    s.feat = dev.denoise(px, cam, pbr.DenoiseParams(passes=1), features=True)[1]
    s.rgba, s.var_out, s.integrated, s.history = dev.denoise_temporal(px, cam, temporal, filt, variance=True, integrated=True, history=True)
    return s


def restate(s, prev, temporal):
    p = None if prev is None else ref.previous(prev.integrated, prev.feat, prev.history[..., 2], prev.cam, prev.px)
    return ref.integrate(s.image, s.var, s.feat, s.cam, s.px, p, temporal)


def check_step(s, prev, temporal, what):
    want_integrated, want_history = restate(s, prev, temporal)
    assert same_values(s.history, want_history), what + " history: " + describe_mismatch(s.history, want_history)
    assert same_values(s.integrated, want_integrated), what + " integrated: " + describe_mismatch(s.integrated, want_integrated)
    return want_integrated, want_history


def usable(s, prev):
    """Pixels whose input and whose own history are finite."""
    return np.isfinite(s.image[..., :3]).all(-1) & np.isfinite(s.var) & np.isfinite(prev.integrated).all(-1)


# ---- 1: the integration, bit for bit ---------------------------------------------------------------------------------

# name -> (BRDF, width, height, temporal parameters, the views of the calls)
MOVE = dict(right=0.35, up=0.1, forward=0.2, turn=0.03)
SEQUENCES = {
    "static-3-calls": (1, W, H, {}, [{}, {}, {}]),
    "moved": (1, W, H, {}, [{}, MOVE, {}]),
    "moved-schlick": (0, W, H, {}, [{}, MOVE]),
    "max-history-2": (1, W, H, dict(max_history=2), [{}, {}, {}, {}]),
    "sigma-world-0": (1, W, H, dict(sigma_world=0.0), [{}, MOVE]),
    "partial-block-72x40": (1, 72, 40, {}, [{}, MOVE]),
}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_integration_is_the_restatement_s_bit_for_bit(pbr, device, name):
    brdf, w, h, tparams, views = SEQUENCES[name]
    sc, cfg, px = cornell(pbr, device, brdf, w, h)
    temporal = pbr.TemporalParams(**tparams)
    prev = None
    for k, move in enumerate(views):
        s = step(pbr, device, px, view(pbr, sc, **move), 100 * k, temporal)
        _, history = check_step(s, prev, temporal, "%s call %d" % (name, k + 1))
        length, valid = history[..., 2], history[..., 3]
        counts = {int(v): int(n) for v, n in zip(*np.unique(length, return_counts=True))}
        print("%s call %d: L %r, pixels with a candidate %.3f, with an accepted tap %.3f" % (name, k + 1, counts, np.isfinite(history[..., 0]).mean(), (valid > 0).mean()))
        # the restatement itself did what the case is about
        if prev is None:
            assert (length == 1).all() and np.isnan(history[..., :2]).all()
        else:
            ok = usable(s, prev)
            assert ok.mean() > 0.99
            if move == views[k - 1]:
                assert (length[ok] == np.minimum(prev.history[..., 2][ok] + 1, temporal.max_history)).all()
                assert (length == min(k + 1, temporal.max_history)).mean() > 0.99
            else:
                fraction = history[..., 0] - np.floor(history[..., 0])
                assert (length[ok] >= 2).mean() > 0.5 and (length[ok] == 1).any()
                assert ((valid == 15) & (fraction > 0.05) & (fraction < 0.95)).mean() > 0.25     # four-tap fetches
            assert np.abs(s.integrated[..., :3][ok] - s.image[..., :3][ok]).max() > 1e-3
        prev = s


# ---- 2: the filter stage ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("passes", [1, 5])
def test_filter_stage_matches_the_numpy_restatement(pbr, device, passes):
    sc, cfg, px = cornell(pbr, device)
    cam = view(pbr, sc)
    filt = pbr.GuidedDenoiseParams(passes=passes)
    step(pbr, device, px, cam, 0, None, filt)
    s = step(pbr, device, px, cam, 100, None, filt)
    assert (s.history[..., 2] == 2).mean() > 0.99                          # the filter's input is a blend
    assert same_values(s.rgba[..., 3], s.image[..., 3])                     # first-hit distance passes through

    given = s.integrated.copy()
    given[..., 3] = s.image[..., 3]
    want, want_var = guided_denoise_ref.guided_numpy(given, s.integrated[..., 3], s.feat, filt, px)
    want64, _ = guided_denoise_ref.guided_numpy(given, s.integrated[..., 3], s.feat, filt, px, exp64=True)
    with np.errstate(invalid="ignore"):
        d = np.abs(want[..., :3] - want64[..., :3])
        spread = float(d[np.isfinite(d)].max())
        err = np.abs(s.rgba[..., :3].astype(np.float64) - want[..., :3])
        err = float(err[np.isfinite(err)].max())
    print("%d passes: D %.3g, colour max |device - restatement| %.3g" % (passes, spread, err))
    assert np.allclose(s.rgba[..., :3], want[..., :3], rtol=2e-5, atol=1e-6 + 4 * spread, equal_nan=True), (err, spread)
    assert np.abs(s.rgba[..., :3] - s.integrated[..., :3]).max() > 1e-3     # ... and it did something
    finite = np.isfinite(s.integrated[..., 3])
    if passes == 1:
        assert np.allclose(s.var_out, want_var, rtol=4e-5, atol=1e-12, equal_nan=True)
    assert np.isfinite(s.var_out[finite]).all() and (s.var_out[finite] >= 0).all()
    assert s.var_out[finite].mean() < s.integrated[..., 3][finite].mean()


def test_without_a_history_the_filter_stage_is_the_guided_filter_s_bit_for_bit(pbr, device):
    """Without a history `integrated` is the guided filter's working plane — {image rgb, variance} (temporal_ref.integrate, prev is
    None) — and both filters run the same passes on the same inputs: same colour, same filtered variance.  One, two and three
    passes end in each of the two output planes."""
    sc, cfg, px = cornell(pbr, device, 1, 72, 40)
    cam = view(pbr, sc)
    image = var = None
    for passes in (1, 2, 3):
        render(pbr, device, px, cam, 0, 4)                                    # a temporal call consumes its render: the same one again
        if image is None:
            image, var = device.read_output(), device.read_variance()
        assert same_values(device.read_output(), image) and same_values(device.read_variance(), var)
        filt = pbr.GuidedDenoiseParams(passes=passes)
        guided, guided_var = device.denoise_guided(px, cam, filt, variance=True)
        device.temporal_reset()
        rgba, var_out, integrated = device.denoise_temporal(px, cam, None, filt, variance=True, integrated=True)
        assert same_values(rgba, guided), "%d passes, rgba: " % passes + describe_mismatch(rgba, guided)
        assert same_values(var_out, guided_var), "%d passes, variance: " % passes + describe_mismatch(var_out, guided_var)
        assert same_values(integrated[..., :3], image[..., :3]) and same_values(integrated[..., 3], var)
        assert np.nanmax(np.abs(rgba[..., :3] - image[..., :3])) > 1e-3      # ... and the passes did something


# ---- 3: disocclusion -------------------------------------------------------------------------------------------------

DISOCCLUDE = dict(right=0.6)


def test_disocclusion_drops_the_history_where_the_surface_was_hidden(pbr, device):
    """A sideways eye move past the boxes: view( right = 0.6 ) — the eye 0.6 units along u (the box is 2 wide, the eye 2.2 to
    4.2 from what it sees), no rotation.  On the device's feature buffers the restatement lets 12.4 % of the hit pixels fall
    back to L = 1 and 87.6 % continue with L = 2 (right = 0.35: 3.8 % / 96.2 %; right = 1.0: 47.8 % / 52.2 %, with little of the
    box left in view)."""
    sc, cfg, px = cornell(pbr, device)
    temporal = pbr.TemporalParams()
    first = step(pbr, device, px, view(pbr, sc), 0, temporal)
    s = step(pbr, device, px, view(pbr, sc, **DISOCCLUDE), 100, temporal)
    _, want = restate(s, first, temporal)
    hit = s.feat[1][..., 3] != 0
    dropped, continued = float((want[..., 2][hit] == 1).mean()), float((want[..., 2][hit] == 2).mean())
    print("disocclusion: of the hit pixels %.3f fall back to L = 1, %.3f continue with L = 2" % (dropped, continued))
    assert dropped >= 0.02 and continued >= 0.50
    assert same_values(s.history[..., 2], want[..., 2]) and same_values(s.history[..., 3], want[..., 3])

    # without the restatement: the heaviest accepted tap of every continued pixel is a point of the previous frame within r
    fx, fy, length, valid = (s.history[..., k] for k in range(4))
    go = hit & (length == 2)
    x0, y0 = np.floor(fx[go]), np.floor(fy[go])
    tx, ty = fx[go] - x0, fy[go] - y0
    best, bx, by = np.zeros(go.sum(), F), np.zeros(go.sum(), np.int64), np.zeros(go.sum(), np.int64)
    for j in range(2):
        for i in range(2):
            bw = (tx if i else F(1.0) - tx) * (ty if j else F(1.0) - ty)
            take = ((valid[go].astype(np.int64) >> (j * 2 + i)) & 1 == 1) & (bw > best)
            best, bx, by = np.where(take, bw, best), np.where(take, x0 + i, bx).astype(np.int64), np.where(take, y0 + j, by).astype(np.int64)
    assert (best > 0).all()
    then, now = first.feat[0][by, bx], s.feat[0][go]
    r = (F(temporal.sigma_world) * F(px)) * now[:, 3]
    assert (ref.sqdist(then, now) <= r * r).all()
    assert (first.feat[2][by, bx][:, 3] == s.feat[2][go][:, 3]).all()       # and of the same material


# ---- 4: it accumulates -----------------------------------------------------------------------------------------------

def test_four_calls_of_four_frames_beat_the_guided_filter_on_four(pbr, device):
    sc, cfg, px = cornell(pbr, device)
    cam = view(pbr, sc)
    temporal = pbr.TemporalParams(max_history=32)
    prev, means, want_means = None, [], []
    for k in range(4):
        s = step(pbr, device, px, cam, 100 * k, temporal, frames=4)
        want_integrated, _ = check_step(s, prev, temporal, "call %d" % (k + 1))
        for into, integ in ((want_means, want_integrated), (means, s.integrated)):
            v = integ[..., 3]
            into.append(float(v[np.isfinite(v)].mean()))
        prev = s
    print("mean integrated variance per call: restatement %r, device %r" % (want_means, means))
    assert want_means[1] < 0.6 * want_means[0]          # the blend gives 0.5 for equal variances
    assert means[1] < 0.6 * means[0]

    guided = device.denoise_guided(px, cam)            # the fourth 4-frame render alone
    device.reset_accum()
    device.render(0, pbr.frame_seeds(1000, 512), px, cam)
    converged = device.read_output()
    ok = np.isfinite(converged[..., :3]).all(-1) & np.isfinite(guided[..., :3]).all(-1) & np.isfinite(s.rgba[..., :3]).all(-1)
    assert ok.mean() > 0.99
    mse = lambda a: float(((a[..., :3] - converged[..., :3])[ok] ** 2).mean())
    print("mse against 512 frames: temporal after 4 x 4 frames %.4g, guided on 4 frames %.4g" % (mse(s.rgba), mse(guided)))
    assert mse(s.rgba) < mse(guided)


# ---- 5: state and arguments ------------------------------------------------------------------------------------------

def test_refusals_by_state(pbr, device):
    sc, cfg, px = cornell(pbr, device, 1, 64, 48)
    cam = view(pbr, sc)
    with pytest.raises(pbr.PbrError, match="pbr_render_adaptive"):        # before any adaptive call
        device.denoise_temporal(px, cam)
    render(pbr, device, px, cam, 0, 4)
    assert device.denoise_temporal(px, cam).shape == (48, 64, 4)
    with pytest.raises(pbr.PbrError, match="pbr_render_adaptive"):        # twice in a row
        device.denoise_temporal(px, cam)
    assert device.denoise_guided(px, cam).shape == (48, 64, 4)             # the guided filter is not bound by that
    device.reset_accum()
    device.render(0, pbr.frame_seeds(0, 2), px, cam)
    with pytest.raises(pbr.PbrError, match="pbr_render_adaptive"):        # after pbr_render
        device.denoise_temporal(px, cam)


def test_tile_sharding_is_refused(pbr, device):
    sc, cfg, px = cornell(pbr, device, 1, 64, 48, tile_world=2, tile_rank=0)
    cam = view(pbr, sc)
    device.render_adaptive(0, pbr.frame_seeds(0, 4), px, cam, 4, 4, 4, 0.0)
    with pytest.raises(pbr.PbrError, match="tile sharding"):
        device.denoise_temporal(px, cam)


@pytest.mark.parametrize("drop", ["temporal_reset", "configure", "upload_scene", "update_vertices"])
def test_the_history_is_dropped(pbr, device, drop):
    sc, cfg, px = cornell(pbr, device, 1, 64, 48)
    cam = view(pbr, sc)
    step(pbr, device, px, cam, 0, frames=4)
    s = step(pbr, device, px, cam, 100, frames=4)
    assert (s.history[..., 2] == 2).mean() > 0.99
    {"temporal_reset": device.temporal_reset, "configure": lambda: device.configure(cfg), "upload_scene": lambda: device.upload_scene(sc.desc),
     "update_vertices": lambda: device.update_vertices(sc.arrays()["vertices"])}[drop]()
    s = step(pbr, device, px, cam, 200, frames=4)
    assert (s.history[..., 2] == 1).all() and np.isnan(s.history[..., :2]).all() and (s.history[..., 3] == 0).all()
    assert same_values(s.integrated[..., :3], s.image[..., :3]) and same_values(s.integrated[..., 3], s.var)
    s = step(pbr, device, px, cam, 300, frames=4)
    assert (s.history[..., 2] == 2).mean() > 0.99                          # ... and it starts again from there


def test_the_history_survives_the_other_filters_and_a_reset_of_the_accumulation(pbr, device):
    sc, cfg, px = cornell(pbr, device, 1, 64, 48)
    cam = view(pbr, sc)
    first = step(pbr, device, px, cam, 0, frames=4)
    device.denoise_guided(px, cam)
    device.denoise(px, cam)
    device.reset_accum()
    s = step(pbr, device, px, cam, 100, frames=4)
    ok = usable(s, first)
    assert ok.mean() > 0.99 and (s.history[..., 2][ok] == 2).all()
    check_step(s, first, pbr.TemporalParams(), "behind the other filters")


def test_argument_errors(pbr, device):
    sc, cfg, px = cornell(pbr, device, 1, 64, 48)
    cam = view(pbr, sc)
    render(pbr, device, px, cam, 0, 4)
    before = device.read_output()
    nan, inf = float("nan"), float("inf")
    bad_temporal = [dict(max_history=0), dict(max_history=1025), dict(normal_cos=-1.5), dict(normal_cos=1.5), dict(normal_cos=nan),
                    dict(sigma_world=-1.0), dict(sigma_world=inf), dict(sigma_world=nan)]
    bad_filter = [dict(passes=0), dict(passes=9), dict(sigma_luminance=-1.0), dict(sigma_world=nan)]
    for bad in bad_temporal:
        with pytest.raises(pbr.PbrError):
            device.denoise_temporal(px, cam, pbr.TemporalParams(**bad))
    for bad in bad_filter:
        with pytest.raises(pbr.PbrError):
            device.denoise_temporal(px, cam, None, pbr.GuidedDenoiseParams(**bad))
    out = np.empty((48, 64, 4), np.float32)
    t, f, o = ctypes.byref(pbr.TemporalParams()), ctypes.byref(pbr.GuidedDenoiseParams()), out.ctypes.data_as(pbr._fp)
    call = pbr.hip.pbr_denoise_temporal
    assert call(device._ctx, px, None, t, f, o, None, None, None) == -1        # PBR_EINVAL
    assert call(device._ctx, px, ctypes.byref(cam), None, f, o, None, None, None) == -1
    assert call(device._ctx, px, ctypes.byref(cam), t, None, o, None, None, None) == -1
    assert call(device._ctx, px, ctypes.byref(cam), t, f, None, None, None, None) == -1
    assert call(None, px, ctypes.byref(cam), t, f, o, None, None, None) == -1
    assert pbr.hip.pbr_temporal_reset(None) == -1
    assert same_values(device.read_output(), before)
    # none of them consumed the render: the call still goes through, as the first one of a history
    out, hist = device.denoise_temporal(px, cam, history=True)
    assert out.shape == (48, 64, 4) and (hist[..., 2] == 1).all() and device.last_kernel_ms() > 0.0


def test_a_call_leaves_the_accumulation_the_moments_and_the_tile_stats_alone(pbr, device):
    sc, cfg, px = cornell(pbr, device, 1, 64, 48)
    cam = view(pbr, sc)
    for k in range(2):
        render(pbr, device, px, cam, 100 * k, 4)
        before, var0, stats = device.read_output(), device.read_variance(), device.tile_stats()
        device.denoise_temporal(px, cam)
        assert same_values(device.read_output(), before)
        assert same_values(device.read_variance(), var0)
        assert all(same_values(a, b) for a, b in zip(device.tile_stats(), stats))


def test_a_refused_call_leaves_no_trace_in_the_history(pbr, device):
    sc, cfg, px = cornell(pbr, device, 1, 64, 48)
    cam, moved = view(pbr, sc), view(pbr, sc, **MOVE)
    results = []
    for with_refusals in (True, False):
        device.temporal_reset()
        step(pbr, device, px, cam, 0, frames=4)
        if with_refusals:
            with pytest.raises(pbr.PbrError):                                # no new render: PBR_ESTATE
                device.denoise_temporal(px, moved)
            render(pbr, device, px, moved, 50, 4)
            with pytest.raises(pbr.PbrError):                                # PBR_EINVAL, with a render waiting
                device.denoise_temporal(px, moved, pbr.TemporalParams(max_history=0))
        results.append(step(pbr, device, px, moved, 100, frames=4))
    a, b = results
    assert same_values(a.history, b.history) and same_values(a.integrated, b.integrated) and same_values(a.rgba, b.rgba)
    assert (a.history[..., 2] == 2).mean() > 0.5
