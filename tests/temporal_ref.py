"""Steps 1 to 4 of pbr_denoise_temporal restated in numpy float32 (include/pbr_hip.h defines them,
physically-based-rendering_amd/csrc/pt_temporal.hpp states them for the device): the candidate, the taps, the history value
and the blend.  Step 5 is guided_denoise_ref.guided_numpy on the result.

Every operation below is one binary32 operation of the device code, in the same order — numpy rounds each float32 product,
sum and quotient on its own, as the library does when built without contraction — so `integrated` and `history` are
reproduced to the bit.  A tap that is left out adds +0 here where the device adds nothing: the sums start at +0 and stay
what they are.

Images are row-major (H, W, 4), row 0 = bottom; features = (position, normal, albedo) as Device.denoise( features=True )
gives them; a camera is anything with .eye / .u / .v / .w that have .x / .y / .z (pbr.Camera), or a dict of 3-vectors.

DECISIONS.  `integrate` (and temporal_motion_ref's) can fill a `Record`: per pixel whether there is a candidate or why not, per
tap that it was used or the first rule in the kernel's order that left it out, which tap gave Hl, blend or which rule made the
pixel a copy, and L.  tests/temporal_planes.py states the same definition in float64 with the same record, and
tests/test_temporal_planes_cpu.py holds the two to the same decisions."""
import types

import numpy as np

F = np.float32

# the candidate of a pixel, in the order the kernel decides
CANDIDATE, BEHIND, LOST, OFF_SCALE = 0, 1, 2, 3
CANDIDATES = {CANDIDATE: "a candidate", LOST: "motion code 3", BEHIND: "!( c > 0 )", OFF_SCALE: "fx or fy not finite"}
# a tap: used, or the first rule that left it out, in the order the kernel decides
USED, NO_CANDIDATE, OUTSIDE, NO_WEIGHT, DIVIDE, MATERIAL, NORMAL, DISTANCE, NOT_FINITE = 0, 1, 2, 3, 4, 5, 6, 7, 8
REASONS = {USED: "used", NO_CANDIDATE: "no candidate", OUTSIDE: "outside the image", NO_WEIGHT: "!( bw > 0 )", DIVIDE: "N'.w != N.w",
           MATERIAL: "A'.w != A.w", NORMAL: "!( dot >= normal_cos )", DISTANCE: "!( distance <= r * r )", NOT_FINITE: "I' not finite"}
# the blend: done, or the first rule that made the pixel a copy of {C, V}
BLENDED, FIRST_CALL, NO_HISTORY, NO_REUSE, INPUT_NOT_FINITE = 0, 1, 2, 3, 4
COPIES = {BLENDED: "blended", FIRST_CALL: "no previous call", NO_HISTORY: "!( S > 0 )", NO_REUSE: "max_history == 1",
          INPUT_NOT_FINITE: "C or V not finite"}


class Record:
    """The decisions of steps 0 to 4 over an (h, w) image."""

    def __init__(self, h, w):
        self.candidate = np.full((h, w), 255, np.uint8)
        self.tap = np.full((h, w, 4), 255, np.uint8)         # j * 2 + i
        self.source = np.full((h, w), -1, np.int64)          # the tap Hl was taken from, -1: none
        self.copy = np.full((h, w), 255, np.uint8)
        self.length = np.zeros((h, w), np.int64)
        self.code = None                                     # the motion path's only: step 0's code, 0 for a miss pixel

    def set_candidate(self, in_front, finite, lost=None):
        """`c > 0 && !lost` is one decision of the kernel: a lost pixel is recorded as LOST whatever its c is (NaN, mostly)."""
        self.candidate[...] = np.where(~in_front, BEHIND, np.where(finite, CANDIDATE, OFF_SCALE))
        if lost is not None:
            self.candidate[lost] = LOST

    def set_tap(self, j, i, has, inside, weight, same_side, hit, material, normal_ok, distance_ok, finite):
        """Tap (j, i) of every pixel; every argument (h, w) bool as the step evaluated it (distance_ok: all True with the term off)."""
        reason = np.full(has.shape, USED, np.uint8)
        for rule, failed in ((NOT_FINITE, ~finite), (DISTANCE, hit & ~distance_ok), (NORMAL, hit & ~normal_ok), (MATERIAL, hit & ~material),
                             (DIVIDE, ~same_side), (NO_WEIGHT, ~weight), (OUTSIDE, ~inside), (NO_CANDIDATE, ~has)):
            reason[failed] = rule
        self.tap[..., j * 2 + i] = reason

    def set_blend(self, weight, reuse, finite, length):
        self.copy[...] = np.where(~weight, NO_HISTORY, np.where(reuse, np.where(finite, BLENDED, INPUT_NOT_FINITE), NO_REUSE))
        self.length[...] = length

    def valid(self):
        """The valid mask as `history` has it."""
        return sum(((self.tap[..., k] == USED).astype(np.int64) << k) for k in range(4))

    def same_decisions(self, other):
        """(h, w) bool"""
        same = (self.candidate == other.candidate) & (self.tap == other.tap).all(-1) & (self.source == other.source)
        same &= (self.copy == other.copy) & (self.length == other.length)
        if self.code is not None or other.code is not None:
            same &= self.code == other.code
        return same


def camera_vectors(cam):
    """-> dict eye / u / v / w of float32 3-vectors."""
    if isinstance(cam, dict):
        return {k: np.asarray(cam[k], F)[:3] for k in ("eye", "u", "v", "w")}
    return {k: np.array([getattr(cam, k).x, getattr(cam, k).y, getattr(cam, k).z], F) for k in ("eye", "u", "v", "w")}


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def sqdist(a, b):
    d = a[..., :3] - b[..., :3]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def previous(integrated, features, lengths, cam, px_dim):
    """What a successful call leaves for the next one."""
    return types.SimpleNamespace(integrated=np.asarray(integrated, F), features=features, lengths=np.asarray(lengths).astype(np.int64),
                                 cam=cam, px_dim=px_dim)


def candidate(features, cam, px_dim, prev_cam, prev_px_dim, record=None):
    """Step 1 -> (fx, fy) float32 (H, W), NaN where there is no candidate.  record: a Record that gets the decision."""
    position, normal, _ = features
    h, w = normal.shape[:2]
    hit = normal[..., 3] != 0
    cur, old = camera_vectors(cam), camera_vectors(prev_cam)
    ys, xs = np.mgrid[0:h, 0:w]
    xs, ys = xs.astype(F)[..., None], ys.astype(F)[..., None]
    with np.errstate(all="ignore"):
        cam_a = cur["u"] - cur["u"] * F(w)                 # setCamera's camA and cvH
        cv_h = cur["v"] * F(h)
        inner = cam_a + cur["u"] * (F(2.0) * xs)
        inner = inner + cur["v"]
        inner = inner - cv_h
        inner = inner + cur["v"] * (F(2.0) * ys)
        d_miss = cur["w"] + inner * (F(px_dim) * F(0.5))
        d_hit = position[..., :3] - old["eye"]
        d = np.where(hit[..., None], d_hit, d_miss).astype(F)
        a = dot(d, old["u"]) / dot(old["u"], old["u"])
        b = dot(d, old["v"]) / dot(old["v"], old["v"])
        c = dot(d, old["w"]) / dot(old["w"], old["w"])
        scale = c * (F(prev_px_dim) * F(0.5))
        fx = (a / scale + F(w - 1)) * F(0.5)
        fy = (b / scale + F(h - 1)) * F(0.5)
        ok = (c > 0) & np.isfinite(fx) & np.isfinite(fy)
        if record is not None:
            record.set_candidate(c > 0, np.isfinite(fx) & np.isfinite(fy))
    nan = F(np.nan)
    return np.where(ok, fx, nan).astype(F), np.where(ok, fy, nan).astype(F)


def integrate(image, var, features, cam, px_dim, prev, params, record=None):
    """Steps 1 to 4.  image (H, W, 4) the accumulation, var (H, W), prev = previous( ... ) or None (the first call after a reset),
    params with .max_history, .normal_cos, .sigma_world -> (integrated (H, W, 4) = {colour, variance}, history (H, W, 4) =
    {fx, fy, L, valid}).  record: a Record that gets the decisions."""
    image, var = np.asarray(image, F), np.asarray(var, F)
    position, normal, albedo = features
    h, w = var.shape
    given = np.concatenate([image[..., :3], var[..., None]], axis=-1).astype(F)
    nan = F(np.nan)
    if prev is None:
        history = np.zeros((h, w, 4), F)
        history[..., 0], history[..., 1], history[..., 2] = nan, nan, F(1.0)
        if record is not None:
            record.candidate[...], record.tap[...], record.copy[...], record.length[...] = BEHIND, NO_CANDIDATE, FIRST_CALL, 1
        return given, history

    fx, fy = candidate(features, cam, px_dim, prev.cam, prev.px_dim, record)
    has = np.isfinite(fx)
    hit = normal[..., 3] != 0
    prev_position, prev_normal, prev_albedo = prev.features
    with np.errstate(all="ignore"):
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0, fy - y0
        radius = (F(params.sigma_world) * F(px_dim)) * position[..., 3]
        radius2 = radius * radius
    acc = np.zeros((h, w, 3), F)
    vsum, wsum, best = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
    length = np.zeros((h, w), np.int64)
    valid = np.zeros((h, w), np.int64)
    for j in range(2):
        for i in range(2):
            with np.errstate(all="ignore"):
                txf, tyf = x0 + F(i), y0 + F(j)
                inside = (txf >= 0) & (txf <= F(w - 1)) & (tyf >= 0) & (tyf <= F(h - 1))
                bw = (tx if i else F(1.0) - tx) * (ty if j else F(1.0) - ty)
                ok = has & inside & (bw > 0)
                xi = np.where(ok, txf, 0).astype(np.int64)
                yi = np.where(ok, tyf, 0).astype(np.int64)
                n, p, a, old = prev_normal[yi, xi], prev_position[yi, xi], prev_albedo[yi, xi], prev.integrated[yi, xi]
                ok &= n[..., 3] == normal[..., 3]
                on_surface = (a[..., 3] == albedo[..., 3]) & (dot(n, normal) >= F(params.normal_cos))
                if F(params.sigma_world) != 0:
                    on_surface &= sqdist(p, position) <= radius2
                ok &= np.where(hit, on_surface, True)
                ok &= np.isfinite(old).all(-1)
                if record is not None:
                    record.set_tap(j, i, has, inside, bw > 0, n[..., 3] == normal[..., 3], hit, a[..., 3] == albedo[..., 3],
                                   dot(n, normal) >= F(params.normal_cos), (F(params.sigma_world) == 0) | (sqdist(p, position) <= radius2),
                                   np.isfinite(old).all(-1))
                acc = acc + np.where(ok[..., None], bw[..., None] * old[..., :3], F(0.0)).astype(F)
                vsum = vsum + np.where(ok, (bw * bw) * old[..., 3], F(0.0)).astype(F)
                wsum = wsum + np.where(ok, bw, F(0.0)).astype(F)
            valid |= np.where(ok, 1 << (j * 2 + i), 0)
            better = ok & (bw > best)
            best = np.where(better, bw, best).astype(F)
            length = np.where(better, prev.lengths[yi, xi], length)
            if record is not None:
                record.source[better] = j * 2 + i

    blend = (wsum > 0) & (int(params.max_history) > 1) & np.isfinite(given).all(-1)
    new_length = np.where(blend, np.minimum(length + 1, int(params.max_history)), 1)
    if record is not None:
        record.set_blend(wsum > 0, int(params.max_history) > 1, np.isfinite(given).all(-1), new_length)
    with np.errstate(all="ignore"):
        hc = acc / wsum[..., None]
        hv = vsum / (wsum * wsum)
        alpha = F(1.0) / new_length.astype(F)
        keep = F(1.0) - alpha
        colour = hc + alpha[..., None] * (given[..., :3] - hc)
        variance = (keep * keep) * hv + (alpha * alpha) * given[..., 3]
    blended = np.concatenate([colour, variance[..., None]], axis=-1).astype(F)
    integrated = np.where(blend[..., None], blended, given).astype(F)
    history = np.stack([fx, fy, new_length.astype(F), valid.astype(F)], axis=-1).astype(F)
    return integrated, history
