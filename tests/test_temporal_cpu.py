"""The numpy restatement of pbr_denoise_temporal's integration (tests/temporal_ref.py) on its own, without a GPU: the
properties the definition in include/pbr_hip.h promises, on synthetic 48 x 32 feature buffers built in numpy — a square
plane at z = 0 facing a lookat camera on the z axis, with sky around it."""
import types

import numpy as np
import pytest

import temporal_ref as ref

F = np.float32
W, H = 48, 32
PX = 0.02
DEPTH = 5.0
HALF = 1.2          # the plane covers |x|, |y| <= HALF: |x| <= 24 * 0.02 * 5 = 2.4 is in view, so there is sky left and right


def params(**kw):
    base = dict(max_history=32, normal_cos=0.9, sigma_world=3.0)
    base.update(kw)
    return types.SimpleNamespace(**base)


def lookat(eye, center, up=(0.0, 1.0, 0.0)):
    """PathTracer::fillCameraBasis: w towards the centre, u = w x up, v = u x w, all normalized."""
    eye, center, up = np.asarray(eye, np.float64), np.asarray(center, np.float64), np.asarray(up, np.float64)
    w = center - eye
    w /= np.linalg.norm(w)
    u = np.cross(w, up)
    u /= np.linalg.norm(u)
    v = np.cross(u, w)
    v /= np.linalg.norm(v)
    return {"eye": eye.astype(F), "u": u.astype(F), "v": v.astype(F), "w": w.astype(F)}


def plane_features(cam, material=2.0):
    """First-hit features of the plane z = 0, |x|, |y| <= HALF, through every pixel centre (float64, rounded once)."""
    c = {k: v.astype(np.float64) for k, v in cam.items()}
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    d = c["w"] + ((2 * xs - (W - 1))[..., None] * c["u"] + (2 * ys - (H - 1))[..., None] * c["v"]) * (PX / 2)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -c["eye"][2] / d[..., 2]
    p = c["eye"] + t[..., None] * d
    hit = (t > 0) & (np.abs(p[..., 0]) <= HALF) & (np.abs(p[..., 1]) <= HALF)
    position = np.zeros((H, W, 4), F)
    position[..., :3] = np.where(hit[..., None], p, 0.0)
    position[..., 3] = np.where(hit, t, np.inf)
    normal = np.zeros((H, W, 4), F)
    normal[hit] = (0, 0, 1, 1)
    albedo = np.zeros((H, W, 4), F)
    albedo[hit] = (0.7, 0.6, 0.5, material)
    albedo[~hit, 3] = -1
    return position, normal, albedo


def noisy(seed, var_value=None):
    rng = np.random.default_rng(seed)
    var = np.full((H, W), var_value, F) if var_value is not None else (rng.uniform(0.001, 0.02, (H, W)) ** 2).astype(F)
    image = np.zeros((H, W, 4), F)
    image[..., :3] = F(0.4) + rng.normal(0, 1, (H, W, 3)).astype(F) * np.sqrt(var)[..., None]
    return image, var


CAM = lookat((0, 0, DEPTH), (0, 0, 0))


@pytest.fixture(scope="module")
def first():
    """The first call: no history.  -> (features, previous)"""
    feat = plane_features(CAM)
    image, var = noisy(1)
    integrated, history = ref.integrate(image, var, feat, CAM, PX, None, params())
    assert np.array_equal(integrated[..., :3], image[..., :3]) and np.array_equal(integrated[..., 3], var)
    assert np.isnan(history[..., :2]).all() and (history[..., 2] == 1).all() and (history[..., 3] == 0).all()
    hit = feat[1][..., 3] != 0
    assert 0.1 < hit.mean() < 0.9                                          # surface and sky are both there
    return feat, ref.previous(integrated, feat, history[..., 2], CAM, PX)


def test_an_identical_camera_reprojects_every_pixel_onto_itself(first):
    feat, _ = first
    fx, fy = ref.candidate(feat, CAM, PX, CAM, PX)
    ys, xs = np.mgrid[0:H, 0:W]
    assert np.isfinite(fx).all() and np.isfinite(fy).all()                 # hit and miss pixels alike
    assert np.abs(fx - xs).max() < 1 / 64 and np.abs(fy - ys).max() < 1 / 64


def test_a_sideways_shift_of_the_eye_moves_fx_by_the_analytic_amount(first):
    """The eye moves by delta along u, the basis stays: a point at depth DEPTH along w was delta / ( DEPTH * PX ) pixels
    further right in the previous image; the sky, at infinity, stays where it is."""
    delta = 0.37
    moved = dict(CAM, eye=(CAM["eye"].astype(np.float64) + delta * CAM["u"]).astype(F))
    feat = plane_features(moved)
    fx, fy = ref.candidate(feat, moved, PX, CAM, PX)
    ys, xs = np.mgrid[0:H, 0:W]
    hit = feat[1][..., 3] != 0
    assert hit.any() and (~hit).any()
    assert np.abs(fx[hit] - (xs[hit] + delta / (DEPTH * PX))).max() < 1 / 64
    assert np.abs(fx[~hit] - xs[~hit]).max() < 1 / 64
    assert np.abs(fy - ys).max() < 1 / 64


@pytest.mark.parametrize("edge", ["material", "normal", "distance"])
def test_a_tap_across_an_edge_is_rejected(first, edge):
    """The previous call's features are changed in the columns x < 24: pixels whose taps all lie there (x <= 22: the taps of a
    static camera are x - 1 .. x + 1) fall back to L = 1 and the input, pixels whose taps all lie at x >= 24 continue."""
    feat, prev = first
    position, normal, albedo = (f.copy() for f in prev.features)
    left = np.zeros((H, W), bool)
    left[:, :24] = True
    hit = feat[1][..., 3] != 0
    if edge == "material":
        albedo[left & hit, 3] = 5
    elif edge == "normal":
        tilt = np.array([np.sin(0.5), 0, np.cos(0.5), 1], F)             # cos 0.878 < 0.9
        normal[left & hit] = tilt
    else:
        position[left & hit, 2] -= F(3.5 * PX * DEPTH)                     # 0.35 > r = 3 * PX * t everywhere: t <= sqrt( 25 + 2 * 1.44 ) = 5.28
        assert (3.5 * PX * DEPTH > 3.0 * PX * position[hit, 3] * 1.01).all()
    changed = ref.previous(prev.integrated, (position, normal, albedo), prev.lengths, CAM, PX)
    image, var = noisy(2)
    integrated, history = ref.integrate(image, var, feat, CAM, PX, changed, params(sigma_world=3.0))
    ys, xs = np.mgrid[0:H, 0:W]
    cut = hit & (xs <= 22)
    kept = hit & (xs >= 25)
    assert cut.any() and kept.any()
    assert (history[cut][:, 3] == 0).all() and (history[cut][:, 2] == 1).all()
    assert np.array_equal(integrated[cut][:, :3], image[cut][:, :3]) and np.array_equal(integrated[cut][:, 3], var[cut])
    assert (history[kept][:, 3] > 0).all() and (history[kept][:, 2] == 2).all()
    assert (history[~hit][:, 2] == 2).all()                                # the sky is not affected by surface features


def test_the_distance_edge_needs_the_distance_term(first):
    """sigma_world = 0 switches the term off: the same shifted history is accepted."""
    feat, prev = first
    position = prev.features[0].copy()
    position[..., 2] -= F(3.5 * PX * DEPTH * 2)
    changed = ref.previous(prev.integrated, (position, prev.features[1], prev.features[2]), prev.lengths, CAM, PX)
    image, var = noisy(2)
    hit = feat[1][..., 3] != 0
    _, on = ref.integrate(image, var, feat, CAM, PX, changed, params())
    _, off = ref.integrate(image, var, feat, CAM, PX, changed, params(sigma_world=0.0))
    assert (on[hit][:, 2] == 1).all() and (off[hit][:, 2] == 2).all()


def test_max_history_1_returns_the_input_bit_for_bit(first):
    feat, prev = first
    image, var = noisy(3)
    integrated, history = ref.integrate(image, var, feat, CAM, PX, prev, params(max_history=1))
    assert np.array_equal(integrated[..., :3], image[..., :3]) and np.array_equal(integrated[..., 3], var)
    assert (history[..., 2] == 1).all()
    assert (history[..., 3] > 0).all()                                     # the taps are still reported


def test_the_history_length_saturates_at_max_history(first):
    feat, prev = first
    for call in range(2, 7):
        image, var = noisy(10 + call)
        integrated, history = ref.integrate(image, var, feat, CAM, PX, prev, params(max_history=3))
        assert (history[..., 2] == min(call, 3)).all(), call
        prev = ref.previous(integrated, feat, history[..., 2], CAM, PX)


def test_a_pixel_without_finite_input_keeps_it_and_starts_over(first):
    feat, prev = first
    image, var = noisy(4)
    var[5, 30], image[6, 31, 1] = np.nan, np.inf
    integrated, history = ref.integrate(image, var, feat, CAM, PX, prev, params())
    assert history[5, 30, 2] == 1 and history[6, 31, 2] == 1 and (np.delete(history[..., 2].ravel(), [5 * W + 30, 6 * W + 31]) == 2).all()
    assert np.isnan(integrated[5, 30, 3]) and np.isinf(integrated[6, 31, 1])
    # ... and such a pixel is no tap for the next call: its neighbours' sums leave it out
    again = ref.previous(integrated, feat, history[..., 2], CAM, PX)
    integrated2, history2 = ref.integrate(*noisy(5), feat, CAM, PX, again, params())
    assert np.isfinite(integrated2).all()


def test_two_calls_of_equal_variance_halve_it(first):
    """alpha = 1 / 2: I.w = Hv / 4 + V / 4 with Hv = sum bw^2 V / ( sum bw )^2.  A static camera's candidate lies within
    e = max |fx - x| of the pixel, the heaviest tap has bw >= ( 1 - e )^2 and the others share the rest, so
    ( 1 - e )^4 <= Hv / V <= 1: the result is V / 2 to a relative 2 e (+ a few ulps of the six operations)."""
    feat, _ = first
    v = 2.5e-4
    image1, var1 = noisy(6, v)
    integrated, history = ref.integrate(image1, var1, feat, CAM, PX, None, params())
    prev = ref.previous(integrated, feat, history[..., 2], CAM, PX)
    image2, var2 = noisy(7, v)
    integrated, history = ref.integrate(image2, var2, feat, CAM, PX, prev, params())
    ys, xs = np.mgrid[0:H, 0:W]
    e = max(float(np.abs(history[..., 0] - xs).max()), float(np.abs(history[..., 1] - ys).max()))
    assert e < 1 / 64
    assert np.allclose(integrated[..., 3], F(v) / 2, rtol=2 * e + 1e-6, atol=0)
    # the colour is the mean of the two renders to the same accuracy of the history fetch
    mean = (image1[..., :3] + image2[..., :3]) / 2
    assert np.abs(integrated[..., :3] - mean).max() < 4 * e * np.abs(image1[..., :3]).max() + 1e-6
