"""The denoise kernels on inputs with known answers (csrc/pt_denoise.hpp, csrc/pt_denoise_guided.hpp).

a. ptd::atrousPass and ptd::atrousGuidedPass through pbr_diag_filter on the planted planes of tests/denoise_ref.py — sizes from
   1 x 1 to 70 x 9 that are no multiple of the 64 x 4 launch block, steps wider than the image, colours, variances and
   distances that are not finite, overflow or underflow — against the definitions of include/pbr_hip.h in float64.  Exact
   where the definition is a decision (what stays, what is not finite, .w), within 4 E_ref + one binary32 ulp where it is a
   value; E_ref is the fp32 restatement's distance from the same truth, measured in this run on the host and never on the
   device (tests/test_filter_planes_cpu.py has the table and the mutants that leave this band).
b. pbr_diag_filter is the public path: pbr_denoise and pbr_denoise_guided equal it on their own inputs, bit for bit.
c. ptd::firstHitFeatures on EVERY pixel of two hand-made scenes whose cameras keep every pixel-centre ray away from edges,
   silhouettes and ties (asserted on the host first): hit or miss, face, material, Kd, normal and its sign, t and position."""
import ctypes

import numpy as np
import pytest

import denoise_ref as R
import hand_scenes
from conftest import same_values, describe_mismatch

pytestmark = pytest.mark.gpu

RUNS = [pytest.param(case, kind, id="%s-%s" % (case.name, ("plain", "guided")[kind])) for case in R.cases() for kind in case.kinds]
MEASURED = {}        # (case name, kind) -> (classes, E_ref colour, device colour, E_ref variance, device variance)


@pytest.fixture(scope="module")
def planes_device(pbr, gpu_device):
    """One context for all of (a): pbr_diag_filter needs it for its device and stream only and leaves it as it was."""
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def params_of(pbr, kind, p):
    if kind == 0:
        return pbr.DenoiseParams(p.passes, p.sigma_color, p.sigma_normal, p.sigma_world, p.sigma_albedo)
    return pbr.GuidedDenoiseParams(p.passes, p.sigma_luminance, p.sigma_normal, p.sigma_world, p.sigma_albedo)


# ---- a: the device against the truth ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case, kind", RUNS)
def test_filter_on_planted_planes_is_the_truth(pbr, planes_device, case, kind):
    p = params_of(pbr, kind, case.params[kind])
    out = planes_device.diag_filter(kind, case.image, case.features, p, float(R.PX_DIM), case.variance if kind == 1 else None)
    rgba, variance = out if kind == 1 else (out, None)
    assert rgba.shape == (case.h, case.w, 4) and rgba.dtype == np.float32
    failures, colour, relative = R.against_truth(case, kind, rgba, variance)
    r = R.evaluate(case, kind)
    MEASURED[(case.name, kind)] = (case.classes, r.e_ref, colour, r.e_ref_variance, relative)
    print("%s kind %d: colour E_ref %.3e device %.3e%s" % (case.name, kind, r.e_ref, colour,
                                                         "" if kind == 0 else "; variance E_ref %.3e device %.3e" % (r.e_ref_variance, relative)))
    assert not failures, failures


def test_measured_errors_per_class():
    """The largest figures of the runs above per class and kind — the table of tests/test_filter_planes_cpu.py."""
    for number, what in sorted(R.CLASSES.items()):
        for kind in (0, 1):
            rows = [v for (name, k), v in MEASURED.items() if k == kind and number in v[0]]
            if rows:
                worst = [max(row[j] for row in rows) if rows[0][j] is not None else None for j in (1, 2, 3, 4)]
                print("class %d %-45s %-6s colour E_ref %.3e device %.3e%s" % (number, what, ("plain", "guided")[kind], worst[0], worst[1],
                      "" if kind == 0 else "  variance E_ref %.3e device %.3e" % (worst[2], worst[3])))


def test_a_refused_call_writes_nothing(pbr, planes_device):
    case = next(c for c in R.cases() if c.name == "neutral_5x3_p1")
    for kind, bad in ((0, dict(passes=0)), (0, dict(passes=9)), (0, dict(sigma_color=-1.0)), (1, dict(sigma_world=float("nan"))), (1, dict(passes=9))):
        p = (pbr.DenoiseParams, pbr.GuidedDenoiseParams)[kind](**bad)
        out, var = np.full((case.h, case.w, 4), 7.0, np.float32), np.full((case.h, case.w), 7.0, np.float32)
        status = pbr.hip.pbr_diag_filter(planes_device._ctx, kind, case.w, case.h, float(R.PX_DIM), ctypes.addressof(p), pbr._as_fp(case.image.copy()),
                                         pbr._as_fp(case.variance.copy()), pbr._as_fp(case.features.copy()), pbr._as_fp(out), pbr._as_fp(var))
        assert status != 0 and (out == 7.0).all() and (var == 7.0).all()
    with pytest.raises(pbr.PbrError):
        planes_device.diag_filter(2, case.image, case.features, pbr.DenoiseParams(), float(R.PX_DIM))
    with pytest.raises(pbr.PbrError):
        planes_device.diag_filter(0, np.zeros((1025, 1024, 4), np.float32), np.zeros((3, 1025, 1024, 4), np.float32), pbr.DenoiseParams(passes=1), 0.01)


# ---- b: the diag entry is the public path --------------------------------------------------------------------------------------

def planted_scene(pbr, dev):
    sc, _, _ = hand_scenes.feature_case(pbr, "wide40")
    dev.upload_scene(sc.desc)
    dev.configure(sc.cfg)
    return sc


def test_pbr_denoise_is_the_diag_filter_on_its_own_planes(pbr, device):
    sc = planted_scene(pbr, device)
    w, h = hand_scenes.FEATURE_W, hand_scenes.FEATURE_H
    rng = np.random.default_rng(5)
    img = rng.uniform(-0.5, 1.5, (h, w, 4)).astype(np.float32)
    img[3, 5, 0], img[4, 6, 1], img[0, 0, 2], img[20, 30, :3], img[21, 30, :3], img[h - 1, w - 1, :3] = np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf
    device.write_input(img)
    device.render_frame(0.0333, 1.0, sc.px, sc.cam)                                   # weight 1: imageOut ~ the injected image
    lin = device.read_output()
    assert np.isnan(lin[3, 5, 0]) and lin[4, 6, 1] == np.inf and np.isnan(lin[20, 30, :3]).all() and (lin[21, 30, :3] == np.inf).all()
    for params in (dict(passes=1), dict(passes=2), dict(passes=5), dict(passes=8), dict(passes=3, sigma_color=0.0),
                   dict(passes=3, sigma_color=0.2, sigma_normal=0.1, sigma_world=1.0, sigma_albedo=0.05)):
        p = pbr.DenoiseParams(**params)
        want, feat = device.denoise(sc.px, sc.cam, p, features=True)
        hit = feat[1][..., 3] != 0
        assert 0.05 < hit.mean() < 0.95
        got = device.diag_filter(0, lin, feat, p, sc.px)
        assert same_values(got, want), "%r: %s" % (params, describe_mismatch(got, want))
        assert same_values(device.read_output(), lin)
    both = np.isfinite(want[..., :3]) & np.isfinite(lin[..., :3])
    assert np.abs(want[..., :3][both] - lin[..., :3][both]).max() > 1e-3


@pytest.mark.parametrize("passes", [1, 3, 5])
def test_pbr_denoise_guided_is_the_diag_filter_on_its_own_planes(pbr, device, passes):
    sc = planted_scene(pbr, device)
    frames = 4
    device.reset_accum()
    device.render_adaptive(0, pbr.frame_seeds(0, frames), sc.px, sc.cam, frames, frames, frames, 0.0)      # a uniform round
    assert (device.tile_stats()[0] == frames).all()
    image, var0 = device.read_output(), device.read_variance()
    assert (var0 > 0).any()
    p = pbr.GuidedDenoiseParams(passes=passes)
    want, want_var, feat = device.denoise_guided(sc.px, sc.cam, p, variance=True, features=True)
    got, got_var = device.diag_filter(1, image, feat, p, sc.px, var0)
    assert same_values(got, want), describe_mismatch(got, want)
    assert same_values(got_var, want_var), describe_mismatch(got_var, want_var)
    assert same_values(device.read_output(), image) and same_values(device.read_variance(), var0)
    assert np.abs(want[..., :3] - image[..., :3])[np.isfinite(want[..., :3])].max() > 1e-4


# ---- c: the feature pass on every pixel --------------------------------------------------------------------------------------------

def feature_case_on_the_host(pbr, shape):
    """The case and what must hold of it before the device is looked at."""
    sc, rays, (t, face, gap, edge) = hand_scenes.feature_case(pbr, shape)
    hit = np.isfinite(t)
    assert same_values(t, hand_scenes.brute_force(sc.arrays["facesV"], sc.arrays["vertices"], rays))
    assert (edge >= hand_scenes.EDGE_MARGIN).all(), int((edge < hand_scenes.EDGE_MARGIN).sum())          # no edge, no silhouette
    assert (gap[hit] > 1e-3 * np.maximum(1.0, t[hit])).all()                                             # no tie: outliers' band
    assert (~hit).mean() >= 0.05 and hit.mean() >= 0.30
    assert set((sc.arrays["facesV"][face[hit], 3]).tolist()) == set(range(len(hand_scenes.FEATURE_KD)))
    assert not sc.flat[face[hit]].any() and sc.arrays["lights"].shape[0] == 0
    return sc, rays, t, face, hit


def check_features(pbr, dev, sc, rays, t, face, hit, feat, what):
    w, h = hand_scenes.FEATURE_W, hand_scenes.FEATURE_H
    position, normal, albedo = (f.reshape(h * w, 4) for f in feat)
    arrays = sc.arrays
    assert ((normal[:, 3] == 1) == hit).all(), "%s: hit / miss differs on %d pixels" % (what, ((normal[:, 3] == 1) != hit).sum())
    # the miss encoding, as the header has it
    assert (position[~hit] == np.array([0, 0, 0, np.inf], np.float32)).all() and not normal[~hit].any()
    assert (albedo[~hit] == np.array([0, 0, 0, -1], np.float32)).all()
    # material and Kd of the brute force's face
    material = arrays["facesV"][face[hit], 3].astype(np.int64)
    assert (albedo[hit][:, 3] == material).all(), "%s: %d materials differ" % (what, (albedo[hit][:, 3] != material).sum())
    assert same_values(albedo[hit][:, :3], arrays["materials"][material, 8:11])
    # the normal: the one pbr_diag_trace reports for the face, turned against the float64 ray
    _, traced_face, traced_normal, _ = dev.diag_trace(rays.astype(np.float32))
    assert (traced_face[hit] == face[hit]).all()
    n = traced_normal[hit].astype(np.float64)
    facing = (n * rays[hit][:, 3:6]).sum(-1)
    assert (np.abs(facing) > 1e-4).all()                                              # no face seen edge-on: the sign is the float64 sign
    want_normal = np.where(facing[:, None] > 0, -traced_normal[hit], traced_normal[hit])
    assert same_values(normal[hit][:, :3], want_normal), "%s normals: %s" % (what, describe_mismatch(normal[hit][:, :3], want_normal))
    assert (normal[hit][:, 3] == 1).all()
    # t and the position within the walk tests' bound of the float64 hit
    assert hand_scenes.outliers(position[:, 3], t).size == 0
    point = rays[hit][:, 0:3] + t[hit][:, None] * rays[hit][:, 3:6]
    assert (np.abs(position[hit][:, :3] - point) <= 1e-3 * np.maximum(1.0, t[hit])[:, None]).all()


@pytest.mark.parametrize("traversal", [0, 2])
@pytest.mark.parametrize("shape", sorted(hand_scenes.FEATURE_CAMERAS))
def test_features_of_every_pixel_are_the_brute_force_s(pbr, device, shape, traversal):
    sc, rays, t, face, hit = feature_case_on_the_host(pbr, shape)
    device.upload_scene(sc.desc)
    device.configure(sc.config(traversal=traversal, arith=0))
    _, feat = device.denoise(sc.px, sc.cam, pbr.DenoiseParams(passes=1), features=True)
    check_features(pbr, device, sc, rays, t, face, hit, feat, "%s, traversal %d" % (shape, traversal))


def test_motion_path_s_face_plane_is_the_brute_force_s(pbr, device):
    """pbr_denoise_temporal behind an update that moves nothing takes the motion path: its face plane is firstHitFeatures'
    faceOut on every pixel."""
    sc, rays, t, face, hit = feature_case_on_the_host(pbr, "wide7")
    w, h, frames = hand_scenes.FEATURE_W, hand_scenes.FEATURE_H, 2
    device.upload_scene(sc.desc)
    device.configure(sc.cfg)
    device.temporal_track_motion(True)
    for k in range(2):
        if k:
            device.update_vertices(sc.arrays["vertices"])
        device.reset_accum()
        device.render_adaptive(0, pbr.frame_seeds(10 * k, frames), sc.px, sc.cam, frames, frames, frames, 0.0)
        device.denoise_temporal(sc.px, sc.cam)
    _, got = device.temporal_motion()
    assert got.shape == (h, w) and (got.reshape(-1) == face).all(), int((got.reshape(-1) != face).sum())
