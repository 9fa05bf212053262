"""The numpy restatement of pbr_read_variance / pbr_denoise_guided (tests/guided_denoise_ref.py) on its own, without a GPU:
the properties the definition in include/pbr_hip.h promises, on synthetic 24 x 16 inputs — a lit wall facing the viewer with a
strip of sky on the right."""
import types

import numpy as np
import pytest

import adaptive_ref
import guided_denoise_ref as ref
from test_gpu_denoise import atrous_numpy

F = np.float32
W, H = 24, 16
PX = 0.01


def params(**kw):
    base = dict(passes=5, sigma_luminance=4.0, sigma_normal=0.25, sigma_world=3.0, sigma_albedo=0.1, sigma_color=0.0)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.fixture(scope="module")
def scene():
    """(image, variance, features): the wall at distance 5 (x < 20), the sky behind it; noise ~ N(0, variance)."""
    rng = np.random.default_rng(7)
    ys, xs = np.mgrid[0:H, 0:W].astype(F)
    hit = xs < 20
    position = np.zeros((H, W, 4), F)
    position[..., 0], position[..., 1], position[..., 2] = xs * F(0.05), ys * F(0.05), F(-5.0)
    position[..., 3] = np.where(hit, F(5.0), F(np.inf))
    position[~hit, :3] = 0
    normal = np.zeros((H, W, 4), F)
    normal[hit] = (0, 0, 1, 1)
    albedo = np.zeros((H, W, 4), F)
    albedo[hit] = (0.7, 0.6, 0.5, 2)
    albedo[~hit, 3] = -1
    var = (rng.uniform(0.001, 0.02, (H, W)) ** 2).astype(F)
    image = np.zeros((H, W, 4), F)
    image[..., :3] = np.where(hit[..., None], F(0.4), F(0.9)) + rng.normal(0, 1, (H, W, 3)).astype(F) * np.sqrt(var)[..., None]
    image[..., 3] = position[..., 3]
    return image, var, (position, normal, albedo)


def test_a_constant_image_is_a_fixed_point(scene):
    image, var, feat = scene
    flat = image.copy()
    flat[..., :3] = (0.3, 0.55, 0.8)
    out, v = ref.guided_numpy(flat, var, feat, params(), PX)
    assert np.allclose(out[..., :3], flat[..., :3], rtol=1e-6, atol=0)
    assert np.array_equal(out[..., 3], flat[..., 3])
    assert np.isfinite(v).all() and (v >= 0).all()


def test_without_variance_a_pixel_that_differs_from_its_neighbours_keeps_its_colour(scene):
    """V_0 = 0: the luminance term is |dY| / 1e-6, and dY >= 0.01 everywhere makes every weight but the centre's 0."""
    image, var, feat = scene
    rng = np.random.default_rng(3)
    steps = image.copy()
    steps[..., :3] = (rng.permutation(W * H).reshape(H, W, 1) * F(0.01)).astype(F)
    out, v = ref.guided_numpy(steps, np.zeros((H, W), F), feat, params(passes=3, sigma_luminance=4.0), PX)
    assert np.allclose(out[..., :3], steps[..., :3], rtol=1e-6, atol=0)
    assert not v.any()


def test_without_the_luminance_term_the_colour_is_the_plain_filter_s(scene):
    image, var, feat = scene
    for passes in (1, 3, 5):
        p = params(passes=passes, sigma_luminance=0.0)
        out, _ = ref.guided_numpy(image, var, feat, p, PX)
        want = atrous_numpy(image, feat, p, PX)          # sigma_color = 0
        assert np.array_equal(out, want)
        assert np.abs(out[..., :3] - image[..., :3]).max() > 1e-3


def test_the_variance_is_the_v_of_the_error_estimate():
    """n0 = 0: M2 / (c - 1) / c is what Moments.error sums — its tiles' errors come out of this variance bit for bit; n0 > 0
    divides by n0 + c instead."""
    rng = np.random.default_rng(11)
    frames = rng.uniform(0, 2, (9, 6, 64, 3)).astype(F)
    m = adaptive_ref.Moments((6, 64))
    for c in range(1, 10):
        m.add(frames[c - 1])
        if c < 2:
            continue
        v = ref.variance(m.m2, c)
        assert v.dtype == F and np.array_equal(v, m.m2 / F(c - 1) / F(c))
        error = np.sqrt(adaptive_ref.butterfly(v) / F(64.0)) / (adaptive_ref.butterfly(m.mean) / F(64.0) + F(0.01))
        assert np.array_equal(error, m.error())
        assert np.array_equal(ref.variance(m.m2, c, 3), m.m2 / F(c - 1) / F(c + 3))
    counts = np.array([4, 4, 8, 9, 9, 8])
    picked = ref.variance_of_frames(frames, counts, [4, 8, 9])
    for t, c in enumerate(counts):
        mt = adaptive_ref.Moments((64,))
        for k in range(c):
            mt.add(frames[k, t])
        assert np.array_equal(picked[t], mt.m2 / F(c - 1) / F(c))


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_tap_whose_variance_is_not_finite_is_left_out(scene, bad):
    """In the pass that meets it such a pixel has no say: whatever colour it holds, every other pixel comes out the same, and
    finite; the pixel itself is filled from its neighbours, variance included, and is a tap like any other from then on."""
    image, var, feat = scene
    y, x = 7, 9
    broken = var.copy()
    broken[y, x] = bad
    other = image.copy()
    other[y, x, :3] = (5.0, 0.0, 7.0)
    p = params(passes=1)
    out_a, v_a = ref.guided_numpy(image, broken, feat, p, PX)
    out_b, v_b = ref.guided_numpy(other, broken, feat, p, PX)
    rest = np.ones((H, W), bool)
    rest[y, x] = False
    assert np.array_equal(out_a[rest], out_b[rest]) and np.array_equal(v_a[rest], v_b[rest])
    assert np.isfinite(out_a[..., :3]).all() and np.isfinite(v_a).all()
    clean, _ = ref.guided_numpy(image, var, feat, p, PX)
    assert not np.array_equal(out_a[y, x + 1], clean[y, x + 1])            # its neighbours do miss it
    out_2, v_2 = ref.guided_numpy(image, broken, feat, params(passes=2), PX)
    assert np.isfinite(out_2[..., :3]).all() and np.isfinite(v_2).all()


def test_a_pass_does_not_raise_the_variance(scene):
    """V_1 = sum w^2 V_0 / ( sum w )^2 <= max V_0 * sum w^2 / ( sum w )^2 <= max V_0 (a few ulps of rounding)."""
    image, var, feat = scene
    for sigma in (0.0, 1.0, 4.0):
        _, v1 = ref.guided_pass(image, var, feat, 1, sigma, 0.25, 3.0, 0.1, PX)
        assert (v1 >= 0).all() and v1.max() <= var.max() * F(1.00001)
        assert v1.mean() < var.mean()


def test_the_float64_exp_variant_is_the_same_filter(scene):
    image, var, feat = scene
    a, va = ref.guided_numpy(image, var, feat, params(), PX)
    b, vb = ref.guided_numpy(image, var, feat, params(), PX, exp64=True)
    assert np.allclose(a, b, rtol=1e-4, atol=1e-6) and np.allclose(va, vb, rtol=0.3, atol=1e-12)
