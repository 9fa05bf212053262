"""pbr_temporal_track_motion / pbr_read_temporal_motion (include/pbr_hip.h, csrc/pt_temporal.hpp): pbr_denoise_temporal's
history across pbr_update_vertices — per-vertex motion.

The motion path (steps 0 to 4 of the header's definition) is a fixed binary32 algorithm: `motion`, `history` and `integrated`
are compared with `same_values` (tolerance 0) against tests/temporal_motion_ref.py, fed with the device's own accumulation,
variance, feature buffers and face plane, the scene's vertex arrays, and the previous call's `integrated` and `history`.

Scene and calls as in test_gpu_temporal.py: HostScene.generate( "cornell", 1, 0 ), render.max_depth 4, 96 x 64 (72 x 40 for
partial blocks), 8 frames per call unless noted, lookat cameras.  What moves is the tall block: the vertices referenced only
by faces of its material, translated by (-0.15, 0, 0) unless noted."""
import types

import numpy as np
import pytest

import temporal_motion_ref as mref
import temporal_ref as ref
from conftest import same_values, describe_mismatch
from test_gpu_temporal import cornell, view, render, usable, MOVE, W, H, FRAMES

pytestmark = pytest.mark.gpu

F = np.float32
BLOCK_MOVE = (-0.15, 0.0, 0.0)
RIGID = (0.25, 0.125, -0.5)
PBR_ESTATE = "-3:"


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def tall_block(arrays):
    """-> (material, vertex mask): the tall block is the only object 1.2 high, and has a material of its own."""
    faces, vertices = arrays["facesV"], arrays["vertices"]
    top = {int(m): float(vertices[faces[faces[:, 3] == m][:, :3].ravel(), 1].max()) for m in np.unique(faces[:, 3])}
    materials = [m for m, y in top.items() if y == float(F(1.2))]
    assert len(materials) == 1, top
    on = faces[:, 3] == materials[0]
    mask = np.zeros(len(vertices), bool)
    mask[faces[on][:, :3].ravel()] = True
    assert mask.any() and not mask[faces[~on][:, :3].ravel()].any()       # non-empty, and shared with no other face
    return materials[0], mask


def translated(vertices, mask, by):
    out = vertices.copy()
    out[mask, :3] = out[mask, :3] + np.asarray(by, F)
    return out


def view_translated(pbr, sc, by, **move):
    """The lookat camera view( ** move ) with its eye translated by `by`: the basis stays what pbrh_camera_lookat gave, bit for bit."""
    out = pbr.Camera.from_buffer_copy(view(pbr, sc, **move))
    e = np.array([out.eye.x, out.eye.y, out.eye.z], F) + np.asarray(by, F)
    out.eye.x, out.eye.y, out.eye.z = float(e[0]), float(e[1]), float(e[2])
    return out


def step(pbr, dev, px, cam, seed0, temporal=None, filt=None, frames=FRAMES, motion=False):
    """One displayed frame as test_gpu_temporal.step, plus the motion step's planes where the call took the motion path."""
    render(pbr, dev, px, cam, seed0, frames)
    s = types.SimpleNamespace(cam=cam, px=px)
    s.image, s.var = dev.read_output(), dev.read_variance()
    s.feat = dev.denoise(px, cam, pbr.DenoiseParams(passes=1), features=True)[1]
    s.rgba, s.var_out, s.integrated, s.history = dev.denoise_temporal(px, cam, temporal, filt, variance=True, integrated=True, history=True)
    if motion:
        s.motion, s.face = dev.temporal_motion()
    return s


def previous(prev):
    return ref.previous(prev.integrated, prev.feat, prev.history[..., 2], prev.cam, prev.px)


def check_motion_step(s, prev, V, Hv, faces, temporal, what):
    want_integrated, want_history, want_motion = mref.integrate(s.image, s.var, s.feat, s.face, V, Hv, faces, s.cam, s.px, previous(prev), temporal)
    assert same_values(s.motion, want_motion), what + " motion: " + describe_mismatch(s.motion, want_motion)
    assert same_values(s.history, want_history), what + " history: " + describe_mismatch(s.history, want_history)
    assert same_values(s.integrated, want_integrated), what + " integrated: " + describe_mismatch(s.integrated, want_integrated)
    return want_integrated, want_history


def lead_taps(history, go):
    """The heaviest accepted tap of the pixels `go` -> (x, y), as test_gpu_temporal's disocclusion test finds it."""
    fx, fy, valid = history[..., 0][go], history[..., 1][go], history[..., 3][go].astype(np.int64)
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = fx - x0, fy - y0
    best, bx, by = np.zeros(fx.size, F), np.zeros(fx.size, np.int64), np.zeros(fx.size, np.int64)
    for j in range(2):
        for i in range(2):
            bw = (tx if i else F(1.0) - tx) * (ty if j else F(1.0) - ty)
            take = ((valid >> (j * 2 + i)) & 1 == 1) & (bw > best)
            best, bx, by = np.where(take, bw, best), np.where(take, x0 + i, bx).astype(np.int64), np.where(take, y0 + j, by).astype(np.int64)
    assert (best > 0).all()
    return bx, by


# ---- 1 + 2: the motion path, bit for bit; static parts untouched ----------------------------------------------------------

# name -> (BRDF, width, height, temporal parameters)
CASES = {
    "sa": (1, W, H, {}),
    "schlick": (0, W, H, {}),
    "partial-block-72x40": (1, 72, 40, {}),
    "sigma-world-0": (1, W, H, dict(sigma_world=0.0)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_motion_path_is_the_restatement_s_bit_for_bit(pbr, device, name):
    """static call; move the tall block; temporal; move it again and the camera (MOVE); temporal."""
    brdf, w, h, tparams = CASES[name]
    sc, cfg, px = cornell(pbr, device, brdf, w, h)
    temporal = pbr.TemporalParams(**tparams)
    arrays = sc.arrays()
    faces, V0 = arrays["facesV"], arrays["vertices"]
    material, mask = tall_block(arrays)
    device.temporal_track_motion(True)
    prev = step(pbr, device, px, view(pbr, sc), 0, temporal)
    with pytest.raises(pbr.PbrError, match=PBR_ESTATE):                     # the static path leaves no motion planes
        device.temporal_motion()
    Hv, full_taps_on_moved_faces = V0, 0
    for k, move in enumerate([{}, MOVE]):
        V = translated(Hv, mask, BLOCK_MOVE)
        device.update_vertices(V)
        s = step(pbr, device, px, view(pbr, sc, **move), 100 * (k + 1), temporal, motion=True)
        what = "%s call %d" % (name, k + 2)
        _, history = check_motion_step(s, prev, V, Hv, faces, temporal, what)
        hit = s.feat[1][..., 3] != 0
        assert ((s.face >= 0) == hit).all() and not s.motion[~hit].any()
        code = s.motion[..., 3]
        on_block = hit & (faces[np.where(hit, s.face, 0), 3] == material)
        assert on_block.any() and (code[on_block] == 2).all() and (code[hit & ~on_block] == 1).all()
        # static parts are untouched: on unmoved faces the candidate is the static definition's, Pprev is P
        fx, fy = ref.candidate(s.feat, s.cam, s.px, prev.cam, prev.px)
        still = hit & ~on_block
        assert same_values(s.history[..., 0][still], fx[still]) and same_values(s.history[..., 1][still], fy[still])
        assert same_values(s.history[..., 0][~hit], fx[~hit]) and same_values(s.motion[..., :3][still], s.feat[0][..., :3][still])
        # the block's points are where they were: Pprev = P - the move, to float32 rounding of the barycentric round trip
        off = np.abs(s.motion[..., :3][on_block] - (s.feat[0][..., :3][on_block] - np.asarray(BLOCK_MOVE, F))).max()
        full = int(((history[..., 3] == 15) & on_block).sum())
        full_taps_on_moved_faces += full
        print("%s: block pixels %d, with L >= 2 %d, with four taps %d, max |Pprev - (P - move)| %.3g" % (what, on_block.sum(), (history[..., 2][on_block] >= 2).sum(), full, off))
        assert off < 1e-5
        ok = usable(s, prev)
        assert ok.mean() > 0.99 and (history[..., 2][ok & on_block] >= 2).mean() > 0.5
        prev, Hv = s, V
    assert full_taps_on_moved_faces > 0


def test_an_update_with_the_same_vertices_is_the_static_definition(pbr, device):
    sc, cfg, px = cornell(pbr, device)
    temporal = pbr.TemporalParams()
    V0 = sc.arrays()["vertices"]
    device.temporal_track_motion(True)
    prev = step(pbr, device, px, view(pbr, sc), 0, temporal)
    device.update_vertices(V0)
    s = step(pbr, device, px, view(pbr, sc, **MOVE), 100, temporal, motion=True)      # the motion path: every face unmoved
    want_integrated, want_history = ref.integrate(s.image, s.var, s.feat, s.cam, s.px, previous(prev), temporal)
    assert same_values(s.history, want_history), describe_mismatch(s.history, want_history)
    assert same_values(s.integrated, want_integrated), describe_mismatch(s.integrated, want_integrated)
    hit = s.feat[1][..., 3] != 0
    assert (s.motion[..., 3][hit] == 1).all() and same_values(s.motion[..., :3][hit], s.feat[0][..., :3][hit])
    assert (want_history[..., 2][usable(s, prev)] >= 2).mean() > 0.5


# ---- 3: tracking on without updates is tracking off ------------------------------------------------------------------------

def test_tracking_without_updates_is_tracking_off(pbr, device):
    results = []
    for on in (False, True):
        sc, cfg, px = cornell(pbr, device)
        device.temporal_track_motion(on)
        calls = [step(pbr, device, px, view(pbr, sc, **move), 100 * k) for k, move in enumerate([{}, MOVE, {}])]
        with pytest.raises(pbr.PbrError, match=PBR_ESTATE):
            device.temporal_motion()
        results.append(calls)
    for a, b in zip(*results):
        assert same_values(a.rgba, b.rgba) and same_values(a.integrated, b.integrated) and same_values(a.history, b.history)
    assert (results[1][1].history[..., 2] >= 2).mean() > 0.5


# ---- 4: rigid translation of everything ------------------------------------------------------------------------------------

@pytest.mark.parametrize("tracked", [True, False])
def test_rigid_translation_of_scene_and_eye(pbr, device, tracked):
    """Every vertex and the eye move by (0.25, 0.125, -0.5): the image is the same, and with per-vertex motion every pixel finds
    itself.  |fx - x|, |fy - y| <= 0.01 is a condition, not a measurement: float32 rounding of P against a pixel footprint is
    about 3e-5 px here, a wrong face or a wrong vertex set is off by at least a pixel.  Without tracking the update drops the
    history: L = 1 everywhere."""
    sc, cfg, px = cornell(pbr, device)
    V0 = sc.arrays()["vertices"]
    V = translated(V0, np.ones(len(V0), bool), RIGID)
    device.temporal_track_motion(tracked)
    prev = step(pbr, device, px, view(pbr, sc), 0)
    device.update_vertices(V)
    s = step(pbr, device, px, view_translated(pbr, sc, RIGID), 100, motion=tracked)
    length = s.history[..., 2]
    if not tracked:
        assert (length == 1).all() and np.isnan(s.history[..., :2]).all()
        return
    hit = (s.feat[1][..., 3] != 0) & usable(s, prev)
    ys, xs = np.mgrid[0:s.var.shape[0], 0:s.var.shape[1]]
    dx, dy = np.abs(s.history[..., 0] - xs)[hit], np.abs(s.history[..., 1] - ys)[hit]
    print("rigid translation: usable hit pixels %d, L = 2 on %.4f, max |fx - x| %.3g, max |fy - y| %.3g" % (hit.sum(), (length[hit] == 2).mean(), dx.max(), dy.max()))
    assert (s.motion[..., 3][hit] == 2).all()
    assert (length[hit] == 2).mean() >= 0.99
    assert dx.max() <= 0.01 and dy.max() <= 0.01


# ---- 5: a moved object and what it uncovers --------------------------------------------------------------------------------

def test_the_moved_block_keeps_its_history_and_what_it_uncovers_starts_over(pbr, device):
    sc, cfg, px = cornell(pbr, device)
    temporal = pbr.TemporalParams()
    arrays = sc.arrays()
    faces, V0 = arrays["facesV"], arrays["vertices"]
    material, mask = tall_block(arrays)
    device.temporal_track_motion(True)
    cam = view(pbr, sc)
    first = step(pbr, device, px, cam, 0, temporal)
    device.update_vertices(translated(V0, mask, BLOCK_MOVE))
    s = step(pbr, device, px, cam, 100, temporal, motion=True)
    length = s.history[..., 2]
    on_block = (s.face >= 0) & (faces[np.where(s.face >= 0, s.face, 0), 3] == material)
    go = on_block & (length == 2)
    was_block = first.feat[2][..., 3] == F(material)
    uncovered = was_block & ~on_block
    print("moved block: %d pixels on it, %.3f continue with L = 2; %d uncovered pixels, %d of them with L = 1" % (
        on_block.sum(), go.sum() / on_block.sum(), uncovered.sum(), (length[uncovered] == 1).sum()))
    assert on_block.sum() > 100 and go.sum() >= 0.5 * on_block.sum()
    bx, by = lead_taps(s.history, go)
    r = (F(temporal.sigma_world) * F(px)) * s.feat[0][go][:, 3]
    assert (ref.sqdist(first.feat[0][by, bx], s.motion[go]) <= r * r).all()
    assert (first.feat[2][by, bx][:, 3] == F(material)).all()
    assert uncovered.sum() > 20 and (length[uncovered] == 1).all()


# ---- 6: two updates equal one ----------------------------------------------------------------------------------------------

def test_two_updates_between_calls_equal_the_last_one(pbr, device):
    results = []
    for twice in (True, False):
        sc, cfg, px = cornell(pbr, device)
        arrays = sc.arrays()
        _, mask = tall_block(arrays)
        device.temporal_track_motion(True)
        step(pbr, device, px, view(pbr, sc), 0)
        if twice:
            device.update_vertices(translated(arrays["vertices"], mask, (0.1, 0.0, 0.05)))
        device.update_vertices(translated(arrays["vertices"], mask, BLOCK_MOVE))
        results.append(step(pbr, device, px, view(pbr, sc, **MOVE), 100, motion=True))
    a, b = results
    for key in ("rgba", "var_out", "integrated", "history", "motion", "face"):
        assert same_values(getattr(a, key), getattr(b, key)), key
    assert (a.motion[..., 3] == 2).any() and (a.history[..., 2] >= 2).mean() > 0.5


# ---- 7: the face plane -----------------------------------------------------------------------------------------------------

def test_the_face_plane_names_the_face_that_was_hit(pbr, device):
    """facesV[face].w is the material in A.w, and P lies on that face: in float64, its distance from the face's plane is at
    most 16 epsilon ( 2^-23 ) times the larger of t and |P|'s largest coordinate — P = origin + t * dir is a handful of binary32
    roundings of numbers that size — and its barycentric coordinates are inside the triangle to 1e-4.  A wrong face is off by
    the distance between two surfaces of the scene (1e-2 at the least) or is another material."""
    sc, cfg, px = cornell(pbr, device, 1, 72, 40)
    arrays = sc.arrays()
    faces, V0 = arrays["facesV"], arrays["vertices"]
    _, mask = tall_block(arrays)
    device.temporal_track_motion(True)
    step(pbr, device, px, view(pbr, sc), 0)
    V = translated(V0, mask, BLOCK_MOVE)
    device.update_vertices(V)
    s = step(pbr, device, px, view(pbr, sc, **MOVE), 100, motion=True)
    hit = s.feat[1][..., 3] != 0
    assert hit.sum() > 500 and ((s.face >= 0) == hit).all() and (s.face[hit] < len(faces)).all()
    f = faces[s.face[hit]]
    assert (f[:, 3].astype(F) == s.feat[2][hit][:, 3]).all()
    a, b, c = (V[f[:, k], :3].astype(np.float64) for k in range(3))
    P = s.feat[0][hit][:, :3].astype(np.float64)
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    distance = np.abs(((P - a) * n).sum(1))
    scale = np.maximum(s.feat[0][hit][:, 3].astype(np.float64), np.abs(P).max(1))
    e1, e2, w = b - a, c - a, P - a
    d11, d12, d22, w1, w2 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1), (w * e1).sum(1), (w * e2).sum(1)
    den = d11 * d22 - d12 * d12
    u, v = (d22 * w1 - d12 * w2) / den, (d11 * w2 - d12 * w1) / den
    print("face plane: %d hit pixels, max distance from the face's plane %.3g (%.2f epsilon of the scale), barycentric overshoot %.3g" % (
        hit.sum(), distance.max(), (distance / (scale * 2.0 ** -23)).max(), max(-u.min(), -v.min(), (u + v - 1).max(), 0.0)))
    assert (distance <= 16 * 2.0 ** -23 * scale).all()
    assert (u >= -1e-4).all() and (v >= -1e-4).all() and (u + v <= 1 + 1e-4).all()


# ---- 8: it accumulates -----------------------------------------------------------------------------------------------------

def test_four_calls_with_a_moving_block_beat_the_guided_filter_on_four_frames(pbr, device):
    sc, cfg, px = cornell(pbr, device)
    arrays = sc.arrays()
    faces, V = arrays["facesV"], arrays["vertices"]
    material, mask = tall_block(arrays)
    cam = view(pbr, sc)
    temporal = pbr.TemporalParams(max_history=32)
    device.temporal_track_motion(True)
    prev, means = None, []
    for k in range(4):
        if k > 0:
            Hv, V = V, translated(V, mask, (-0.05, 0.0, 0.0))
            device.update_vertices(V)
        s = step(pbr, device, px, cam, 100 * k, temporal, frames=4, motion=k > 0)
        on_block = s.feat[2][..., 3] == F(material)
        if k > 0:
            check_motion_step(s, prev, V, Hv, faces, temporal, "call %d" % (k + 1))
            on_block &= s.history[..., 2] >= 2
        v = s.integrated[..., 3][on_block]
        means.append(float(v[np.isfinite(v)].mean()))
        prev = s
    print("mean integrated variance on the block per call: %r" % means)
    assert means[1] < 0.6 * means[0]                      # the blend gives 0.5 for equal variances

    guided = device.denoise_guided(px, cam)              # the fourth 4-frame render alone
    device.reset_accum()
    device.render(0, pbr.frame_seeds(1000, 512), px, cam)
    converged = device.read_output()
    ok = np.isfinite(converged[..., :3]).all(-1) & np.isfinite(guided[..., :3]).all(-1) & np.isfinite(s.rgba[..., :3]).all(-1)
    assert ok.mean() > 0.99
    mse = lambda a: float(((a[..., :3] - converged[..., :3])[ok] ** 2).mean())
    print("mse against 512 frames: temporal after 4 x 4 frames with the block moving %.4g, guided on 4 frames %.4g" % (mse(s.rgba), mse(guided)))
    assert mse(s.rgba) < mse(guided)


# ---- 9: state --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("drop", ["temporal_reset", "configure", "upload_scene", "update_untracked"])
def test_the_history_is_dropped_with_tracking_on(pbr, device, drop):
    sc, cfg, px = cornell(pbr, device, 1, 64, 48)
    arrays = sc.arrays()
    _, mask = tall_block(arrays)
    moved = translated(arrays["vertices"], mask, BLOCK_MOVE)
    cam = view(pbr, sc)
    device.temporal_track_motion(True)
    step(pbr, device, px, cam, 0, frames=4)
    device.update_vertices(moved)
    s = step(pbr, device, px, cam, 100, frames=4, motion=True)
    assert (s.history[..., 2] == 2).mean() > 0.8

    def update_untracked():
        device.temporal_track_motion(False)
        device.update_vertices(arrays["vertices"])

    {"temporal_reset": device.temporal_reset, "configure": lambda: device.configure(cfg), "upload_scene": lambda: device.upload_scene(sc.desc),
     "update_untracked": update_untracked}[drop]()
    if drop == "configure":
        with pytest.raises(pbr.PbrError, match=PBR_ESTATE):                 # the planes went with the images
            device.temporal_motion()
    s = step(pbr, device, px, cam, 200, frames=4)
    assert (s.history[..., 2] == 1).all() and np.isnan(s.history[..., :2]).all() and (s.history[..., 3] == 0).all()
    assert same_values(s.integrated[..., :3], s.image[..., :3]) and same_values(s.integrated[..., 3], s.var)
    if drop != "update_untracked":                                          # the flag itself survived: the next update keeps the history
        device.update_vertices(moved)
        s = step(pbr, device, px, cam, 300, frames=4, motion=True)
        assert (s.history[..., 2] == 2).mean() > 0.8


def test_turning_tracking_off_after_a_move_drops_the_history(pbr, device):
    sc, cfg, px = cornell(pbr, device, 1, 64, 48)
    arrays = sc.arrays()
    _, mask = tall_block(arrays)
    cam = view(pbr, sc)
    device.temporal_track_motion(True)
    step(pbr, device, px, cam, 0, frames=4)
    device.temporal_track_motion(False)                                     # no move yet: the history is the current geometry's
    device.temporal_track_motion(True)
    s = step(pbr, device, px, cam, 100, frames=4)
    assert (s.history[..., 2] == 2).mean() > 0.99
    device.update_vertices(translated(arrays["vertices"], mask, BLOCK_MOVE))
    device.temporal_track_motion(False)
    s = step(pbr, device, px, cam, 200, frames=4)
    assert (s.history[..., 2] == 1).all()


def test_a_call_on_the_motion_path_leaves_the_rest_of_the_context_alone(pbr, device):
    sc, cfg, px = cornell(pbr, device, 1, 64, 48)
    arrays = sc.arrays()
    _, mask = tall_block(arrays)
    cam = view(pbr, sc)
    device.temporal_track_motion(True)
    step(pbr, device, px, cam, 0, frames=4)
    device.update_vertices(translated(arrays["vertices"], mask, BLOCK_MOVE))
    render(pbr, device, px, cam, 100, 4)
    before, var0, stats, bvh, info = device.read_output(), device.read_variance(), device.tile_stats(), device.read_bvh(), device.refit_info()
    device.denoise_temporal(px, cam)
    device.temporal_motion()
    assert same_values(device.read_output(), before) and same_values(device.read_variance(), var0)
    assert all(same_values(a, b) for a, b in zip(device.tile_stats(), stats))
    assert same_values(device.read_bvh(), bvh)
    after = device.refit_info()
    assert after["device_bytes"] == info["device_bytes"] and after["updates"] == info["updates"]   # H is not part of refitBytes


def test_refused_calls_leave_no_trace(pbr, device):
    sc, cfg, px = cornell(pbr, device, 1, 64, 48)
    arrays = sc.arrays()
    _, mask = tall_block(arrays)
    moved = translated(arrays["vertices"], mask, BLOCK_MOVE)
    cam, other = view(pbr, sc), view(pbr, sc, **MOVE)
    device.temporal_track_motion(True)
    results = []
    for with_refusals in (True, False):
        device.update_vertices(arrays["vertices"])
        device.temporal_reset()
        step(pbr, device, px, cam, 0, frames=4)
        device.update_vertices(moved)
        if with_refusals:
            with pytest.raises(pbr.PbrError):                                # no new render: PBR_ESTATE
                device.denoise_temporal(px, other)
            render(pbr, device, px, other, 50, 4)
            with pytest.raises(pbr.PbrError):                                # PBR_EINVAL, with a render waiting
                device.denoise_temporal(px, other, pbr.TemporalParams(max_history=0))
            with pytest.raises(pbr.PbrError):                                # a refused update: wrong vertex count
                device.update_vertices(moved[:-1])
            with pytest.raises(pbr.PbrError, match=PBR_ESTATE):             # no call has taken the motion path yet
                device.temporal_motion()
        results.append(step(pbr, device, px, other, 100, frames=4, motion=True))
    a, b = results
    for key in ("rgba", "integrated", "history", "motion", "face"):
        assert same_values(getattr(a, key), getattr(b, key)), key
    assert (a.history[..., 2] == 2).mean() > 0.5 and (a.motion[..., 3] == 2).any()
