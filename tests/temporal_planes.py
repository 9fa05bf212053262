"""Steps 0 to 4 of pbr_denoise_temporal on planted histories: the cases, and the definition in float64.

  temporal_ref.integrate, temporal_motion_ref.integrate   the fp32 RESTATEMENTS: every operation one binary32 operation of
                                                          the device code (csrc/pt_temporal.hpp), in its order
  motion_truth64, integrate_truth64                       the TRUTH: the definition in include/pbr_hip.h with every value in
                                                          float64 — differences, dot products, quotients, sqrt, sums, blend

The truth takes the float32 inputs as given.  It follows binary32 only where the definition names a binary32 DECISION:
  * "not finite" of a computed quantity — fx, fy in step 1; u, v, Pprev in step 0 — is binary32's: the quantity is a binary32
    one, its infinity starts at 2^128 - 2^103.  The truth rounds its float64 value to binary32 and asks there.  So a candidate
    8e30 pixels away is one (and has no tap), and one at 1e40 is none;
  * "not finite" of C, V and I', the equality of the nine coordinates that makes a face unmoved, N'.w == N.w and A'.w == A.w
    are asked of the inputs, which are binary32;
  * L = min( Hl + 1, max_history ) is integer arithmetic (the kernel's 32-bit unsigned, here int64: the same for Hl in
    1 .. 1024, which is all pbr_diag_temporal admits), alpha = 1 / L.
Every comparison — c > 0, inside the image, bw > 0, dot >= normal_cos * len, distance <= r * r, dot( N, n ) < 0, S > 0, the
largest bw — is made on the float64 values.  The cases are planted so that both sides decide alike on every pixel: thresholds
are hit exactly with dyadic inputs (both arithmetics are exact there), everything else has margin.
What the truth does NOT follow: an intermediate that overflows binary32 while the definition's value is finite (Hc + alpha *
( C - Hc ) near FLT_MAX; a cross product of edges near 1e38).  There the restatement, like the device, stores inf or NaN and the
truth a finite value; those pixels are counted per class (`apart`) and left out of E_ref.  Device and restatement still have
to agree on them bit for bit.

CASES.  `cases()` is the one table, seeded (SEED).  Most cases use axis-aligned cameras, pxDim = 2^-5 and a plane at depth 4
with dyadic eye positions, so that a, b, c, fx, fy, bw, r * r and the dot products are exact in binary32.  `CLASSES` names
the classes; a case carries `pairs` — (what, accepted pixel, rejected pixel, tap, the rule that rejects) — for every
threshold it plants on both sides."""
import functools
import types

import numpy as np

import temporal_motion_ref as mref
import temporal_ref as ref

F, D = np.float32, np.float64
SEED = 41
PX = F(2.0 ** -5)
DEPTH = 4.0
W, H = 7, 5
SIZES = ((1, 1), (2, 2), (7, 5), (64, 4), (65, 5), (70, 9))
CLASSES = {1: "sizes", 2: "candidates", 3: "tap tests", 4: "blend", 5: "miss pixels", 6: "motion"}


def ulp32(x):
    """The spacing of binary32 at |x| (float64 in, float64 out; the smallest subnormal below 2^-126)."""
    x = np.abs(np.asarray(x, D))
    with np.errstate(all="ignore"):
        e = np.floor(np.log2(np.where(x > 0, x, 1.0)))
    return np.where(x > 0, np.exp2(np.maximum(e, -126.0) - 23.0), 2.0 ** -149)


def finite32(x):
    """Is the float64 quantity finite once it is the binary32 quantity the definition speaks of?"""
    with np.errstate(all="ignore"):
        return np.isfinite(np.asarray(x, D).astype(F))


# ---- cameras and planes ---------------------------------------------------------------------------------------------------

def camera(eye=(0, 0, 0), u=(1, 0, 0), v=(0, 1, 0), w=(0, 0, -1)):
    return {"eye": np.array(eye, F), "u": np.array(u, F), "v": np.array(v, F), "w": np.array(w, F)}


def lookat(eye, target, up=(0, 1, 0)):
    """u = w x up, v = u x w, all normalized: what PathTracer::fillCameraBasis hands out, rounded to binary32."""
    eye, target, up = (np.array(a, D) for a in (eye, target, up))
    w = (target - eye) / np.linalg.norm(target - eye)
    u = np.cross(w, up)
    u /= np.linalg.norm(u)
    return camera(eye, u, np.cross(u, w), w)


def centre_directions(cam, px, w, h):
    """centreRay's direction before normalize, float64 (h, w, 3)."""
    c = {k: np.asarray(x, D) for k, x in cam.items()}
    ys, xs = np.mgrid[0:h, 0:w].astype(D)
    inner = c["u"] * (2 * xs - (w - 1))[..., None] + c["v"] * (2 * ys - (h - 1))[..., None]
    return c["w"] + inner * (float(px) / 2)


def plane_features(cam, px, w, h, depth=DEPTH, t=DEPTH, material=2.0):
    """What the pixel centres of `cam` see of the plane z = -depth: position {x, y, z, t}, normal {0, 0, 1, 1}, albedo
    {.5, .5, .5, material}.  t: the planted first-hit distance, None = the ray's length.  Exact
    for an axis-aligned camera with a dyadic eye."""
    d = centre_directions(cam, px, w, h)
    s = (-depth - float(cam["eye"][2])) / d[..., 2]
    position = np.zeros((h, w, 4), F)
    position[..., :3] = np.asarray(cam["eye"], D) + d * s[..., None]
    position[..., 3] = t if t is not None else np.linalg.norm(d, axis=-1) * s
    normal, albedo = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    normal[...] = (0, 0, 1, 1)
    albedo[...] = (0.5, 0.5, 0.5, material)
    return [position, normal, albedo]


def make_miss(features, where):
    """firstHitFeatures' miss pixel."""
    features[0][where] = (0, 0, 0, np.inf)
    features[1][where] = 0
    features[2][where] = (0, 0, 0, -1)


def shifted(sx, sy):
    """The camera whose pixel (x, y) sees what the camera at the origin sees at (x + sx, y + sy), pixels of PX at DEPTH."""
    return camera((sx * DEPTH * float(PX), sy * DEPTH * float(PX), 0))


def params(max_history=32, normal_cos=0.5, sigma_world=2.0):
    return types.SimpleNamespace(max_history=max_history, normal_cos=normal_cos, sigma_world=sigma_world)


# ---- the truth ----------------------------------------------------------------------------------------------------------------

def dot64(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def motion_truth64(features, face, vertices, hist_vertices, faces_v, record=None):
    """Step 0 in float64 -> types.SimpleNamespace( motion (h, w, 4) {Pprev, code}, reference (h, w, 4) {nref, len}, float64, and the
    terms the error bounds of tests/test_temporal_planes_cpu.py are made of )."""
    position, normal, _ = (np.asarray(f, D) for f in features)
    face = np.asarray(face)
    V, Hv = np.asarray(vertices, D), np.asarray(hist_vertices, D)
    hit = face >= 0
    corners = np.asarray(faces_v)[np.where(hit, face, 0)].astype(np.int64)
    a, b, c = (V[corners[..., k]][..., :3] for k in range(3))
    a2, b2, c2 = (Hv[corners[..., k]][..., :3] for k in range(3))
    unmoved = (a == a2).all(-1) & (b == b2).all(-1) & (c == c2).all(-1)
    P, N = position[..., :3], normal[..., :3]
    with np.errstate(all="ignore"):
        e1, e2, w = b - a, c - a, P - a
        d11, d12, d22 = dot64(e1, e1), dot64(e1, e2), dot64(e2, e2)
        w1, w2 = dot64(w, e1), dot64(w, e2)
        den = d11 * d22 - d12 * d12
        u = (d22 * w1 - d12 * w2) / den
        v = (d11 * w2 - d12 * w1) / den
        e1p, e2p = b2 - a2, c2 - a2
        pprev = a2 + e1p * u[..., None] + e2p * v[..., None]
        n, n2 = np.cross(e1, e2), np.cross(e1p, e2p)
        n2 = np.where((dot64(N, n) < 0)[..., None], -n2, n2)
        length = np.sqrt(dot64(n2, n2))
        # |u|, |v| with the cancellation in their numerators and in den undone: what an error in them is relative to
        spread = (d11 * d22 + d12 * d12) / np.abs(den)
        u_size = (np.abs(d22 * w1) + np.abs(d12 * w2)) / np.abs(den) * spread
        v_size = (np.abs(d11 * w2) + np.abs(d12 * w1)) / np.abs(den) * spread
    finite = finite32(u) & finite32(v) & finite32(pprev).all(-1)
    code = np.where(hit, np.where(unmoved, 1.0, np.where(finite, 2.0, 3.0)), 0.0)
    moved = np.concatenate([np.where(unmoved[..., None], P, pprev), code[..., None]], -1)
    reference = np.concatenate([np.where(unmoved[..., None], N, n2), np.where(unmoved, 1.0, length)[..., None]], -1)
    moved[~hit], reference[~hit] = 0, 0
    if record is not None:
        record.code = code.astype(np.uint8)
    return types.SimpleNamespace(motion=moved, reference=reference, unmoved=unmoved | ~hit, u=u, v=v, u_size=u_size, v_size=v_size,
                                 a2=a2, e1p=e1p, e2p=e2p)


def integrate_truth64(case, record=None):
    """Steps 0 to 4 in float64 -> types.SimpleNamespace( integrated (h, w, 4), fx, fy (h, w; NaN: no candidate), length (h, w) int64,
    valid (h, w) int64, step0 = motion_truth64's or None, and the terms of the error bounds )."""
    image, var = np.asarray(case.image, D), np.asarray(case.variance, D)
    position, normal, albedo = (np.asarray(f, D) for f in case.features)
    h, w = var.shape
    p = case.params
    given = np.concatenate([image[..., :3], var[..., None]], -1)
    out = types.SimpleNamespace(step0=None)
    if case.prev is None:
        if record is not None:
            record.candidate[...], record.tap[...], record.copy[...], record.length[...] = ref.BEHIND, ref.NO_CANDIDATE, ref.FIRST_CALL, 1
        out.integrated, out.fx, out.fy = given, np.full((h, w), np.nan), np.full((h, w), np.nan)
        out.length, out.valid = np.ones((h, w), np.int64), np.zeros((h, w), np.int64)
        out.largest = np.abs(given)
        out.fx_scale = np.zeros((h, w))
        return out
    prev = case.prev
    hit = normal[..., 3] != 0
    p_ref, n_ref, bound = position, normal, np.full((h, w), float(F(p.normal_cos)))
    lost = np.zeros((h, w), bool)
    if case.motion is not None:
        m = case.motion
        out.step0 = motion_truth64(case.features, m.face, m.vertices, m.hist_vertices, m.faces_v, record)
        p_ref = np.where(hit[..., None], out.step0.motion, position)
        n_ref = np.where(hit[..., None], out.step0.reference, normal)
        bound = np.where(hit, float(F(p.normal_cos)) * out.step0.reference[..., 3], bound)
        lost = hit & (out.step0.motion[..., 3] == 3)

    # 1. the candidate
    cur, old = ({k: np.asarray(x, D) for k, x in ref.camera_vectors(c).items()} for c in (case.cam, prev.cam))
    half, old_half = float(F(case.px_dim) * F(0.5)), float(F(prev.px_dim) * F(0.5))
    with np.errstate(all="ignore"):
        d = np.where(hit[..., None], p_ref[..., :3] - old["eye"], centre_directions(cur, 2 * half, w, h))
        a, b, c = (dot64(d, old[k]) / dot64(old[k], old[k]) for k in ("u", "v", "w"))
        scale = c * old_half
        fx = (a / scale + (w - 1)) * 0.5
        fy = (b / scale + (h - 1)) * 0.5
        in_front, finite = c > 0, finite32(fx) & finite32(fy)
        # sum | terms | of the three dot products over | their denominators |: what an error in a / scale is relative to
        size = lambda k: (np.abs(d) * np.abs(old[k])).sum(-1) / dot64(old[k], old[k])
        out.fx_largest = np.maximum(np.maximum(size("u"), size("v")) / np.abs(scale) * np.maximum(1.0, size("w") / np.abs(c)), max(w, h) - 1)
        out.fx_per_world = np.maximum.reduce([np.abs(old[k]).max() / dot64(old[k], old[k]) for k in ("u", "v", "w")]) / np.abs(scale) \
            * (1 + np.maximum(np.abs(a), np.abs(b)) / np.abs(c))
    has = in_front & finite & ~lost
    if record is not None:
        record.set_candidate(in_front, finite, lost)
    out.fx, out.fy = np.where(has, fx, np.nan), np.where(has, fy, np.nan)

    # 2. the taps, 3. the history
    prev_position, prev_normal, prev_albedo = (np.asarray(f, D) for f in prev.features)
    prev_i = np.asarray(prev.integrated, D)
    prev_i_finite = np.isfinite(np.asarray(prev.integrated, F)).all(-1)
    with np.errstate(all="ignore"):
        x0, y0 = np.floor(out.fx), np.floor(out.fy)
        tx, ty = out.fx - x0, out.fy - y0
        radius = (float(F(p.sigma_world)) * float(F(case.px_dim))) * position[..., 3]
        radius2 = radius * radius
    acc, vsum, wsum, best = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
    length, valid = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    largest = np.abs(given)
    for j in range(2):
        for i in range(2):
            with np.errstate(all="ignore"):
                txf, tyf = x0 + i, y0 + j
                inside = (txf >= 0) & (txf <= w - 1) & (tyf >= 0) & (tyf <= h - 1)
                bw = (tx if i else 1 - tx) * (ty if j else 1 - ty)
                reach = has & inside & (bw > 0)
                xi, yi = np.where(reach, txf, 0).astype(np.int64), np.where(reach, tyf, 0).astype(np.int64)
                n, q, al, old_i = prev_normal[yi, xi], prev_position[yi, xi], prev_albedo[yi, xi], prev_i[yi, xi]
                same_side, material = n[..., 3] == normal[..., 3], al[..., 3] == albedo[..., 3]
                normal_ok = dot64(n, n_ref) >= bound
                delta = q[..., :3] - p_ref[..., :3]
                distance_ok = (dot64(delta, delta) <= radius2) if float(F(p.sigma_world)) != 0 else np.ones((h, w), bool)
                finite_i = prev_i_finite[yi, xi]
                ok = reach & same_side & np.where(hit, material & normal_ok & distance_ok, True) & finite_i
                acc = acc + np.where(ok[..., None], bw[..., None] * old_i[..., :3], 0.0)
                vsum = vsum + np.where(ok, (bw * bw) * old_i[..., 3], 0.0)
                wsum = wsum + np.where(ok, bw, 0.0)
                largest = np.where(ok[..., None], np.maximum(largest, np.abs(old_i)), largest)
            if record is not None:
                record.set_tap(j, i, has, inside, bw > 0, same_side, hit, material, normal_ok, distance_ok, finite_i)
            valid |= np.where(ok, 1 << (j * 2 + i), 0)
            better = ok & (bw > best)
            best = np.where(better, bw, best)
            length = np.where(better, prev.lengths[yi, xi], length)
            if record is not None:
                record.source[better] = j * 2 + i

    # 4. the blend
    given_finite = np.isfinite(np.asarray(given, F)).all(-1)
    blend = (wsum > 0) & (int(p.max_history) > 1) & given_finite
    new_length = np.where(blend, np.minimum(length + 1, int(p.max_history)), 1)
    if record is not None:
        record.set_blend(wsum > 0, int(p.max_history) > 1, given_finite, new_length)
    with np.errstate(all="ignore"):
        hc, hv = acc / wsum[..., None], vsum / (wsum * wsum)
        alpha = 1.0 / new_length
        colour = hc + alpha[..., None] * (given[..., :3] - hc)
        variance = ((1 - alpha) * (1 - alpha)) * hv + (alpha * alpha) * given[..., 3]
    blended = np.concatenate([colour, variance[..., None]], -1)
    out.integrated = np.where(blend[..., None], blended, given)
    out.length, out.valid, out.blend, out.largest, out.weight = new_length, valid, blend, largest, wsum
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------

class Case:
    """One planted call.  image (h, w, 4), variance (h, w), features [position, normal, albedo], cam, px_dim, params; prev =
    temporal_ref.previous( ... ) or None; motion = None or a namespace face / vertices / hist_vertices / faces_v."""

    def __init__(self, name, classes, w, h, cam, prev_cam, rng, px_dim=PX, prev_px_dim=PX, p=None, t=DEPTH, first_call=False):
        self.name, self.classes, self.w, self.h = name, set(classes), w, h
        self.cam, self.px_dim, self.params = cam, px_dim, p or params()
        self.features = plane_features(cam, px_dim, w, h, t=t)
        self.image = rng.uniform(0.1, 1.0, (h, w, 4)).astype(F)
        self.variance = rng.uniform(1e-4, 1e-2, (h, w)).astype(F)
        self.motion, self.pairs = None, []
        self.may_overflow = np.zeros((h, w), bool)       # pixels where an intermediate may overflow binary32 alone: see the docstring
        self.prev = None
        if not first_call:
            integrated = rng.uniform(0.1, 1.0, (h, w, 4)).astype(F)
            integrated[..., 3] = rng.uniform(1e-4, 1e-2, (h, w))
            lengths = (np.arange(h * w).reshape(h, w) * 7 % 31 + 1).astype(np.int64)          # distinct among neighbours
            self.prev = ref.previous(integrated, plane_features(prev_cam, prev_px_dim, w, h, t=t), lengths, prev_cam, prev_px_dim)

    def pair(self, what, accepted, rejected, rule, tap=0):
        self.pairs.append((what, accepted, rejected, tap, rule))


def _candidate_cases(rng, add):
    origin = camera()
    shifts = {"same": (0, 0), "qx": (0.25, 0), "hx": (0.5, 0), "qy": (0, 0.25), "hy": (0, 0.5), "qxy": (0.25, 0.25), "hxy": (0.5, 0.5),
              "hx_back": (-0.5, 0), "hy_back": (0, -0.5), "hxy_back": (-0.5, -0.5), "q_mixed": (0.75, -0.25), "whole_image": (W, 0),
              "whole_image_y": (0, -H), "almost_whole": (W - 0.5, 0)}
    for name, (sx, sy) in shifts.items():
        add(Case("shift_" + name, {2}, W, H, shifted(sx, sy), origin, rng, p=params(sigma_world=0.0 if "whole" in name else 2.0)))
    add(Case("c_zero", {2}, W, H, origin, camera((0, 0, -DEPTH)), rng))
    add(Case("c_negative", {2}, W, H, origin, camera(u=(-1, 0, 0), w=(0, 0, 1)), rng))
    add(Case("eye_1e30", {2}, W, H, origin, camera((1e30, 0, 0)), rng))
    # c = 2^-140: scale = 2^-146 is a subnormal, a / scale overflows binary32 unless a == 0 (the middle column and row)
    case = Case("c_subnormal", {2}, W, H, origin, origin, rng, p=params(sigma_world=0.0))
    case.features[0][..., :2] *= F(2.0 ** -10)
    case.features[0][..., 2] = -2.0 ** -140
    add(case)
    case = Case("nan_in_p", {2}, W, H, shifted(0.5, 0), origin, rng)
    case.features[0][2, 3, 0], case.features[0][1, 1, 1], case.features[0][3, 5, 2] = np.nan, np.nan, np.inf
    case.features[0][1, 4, 3], case.features[0][3, 2, 3] = np.nan, np.inf                    # t: r is NaN / inf, the candidate stays
    add(case)
    add(Case("basis_not_orthogonal", {2}, W, H, shifted(0.25, 0.5), camera(u=(1, 0.25, 0), v=(0.125, 1, 0)), rng))
    add(Case("basis_not_unit", {2}, W, H, shifted(0.5, 0.25), camera(u=(2, 0, 0), v=(0, 0.5, 0), w=(0, 0, -4)), rng))
    add(Case("px_dim_doubled", {2}, W, H, shifted(0.5, 0), origin, rng, prev_px_dim=F(2.0 ** -4)))
    add(Case("px_dim_halved", {2}, W, H, origin, origin, rng, prev_px_dim=F(2.0 ** -6), p=params(sigma_world=0.0)))
    add(Case("lookat_pair", {2}, W, H, lookat((0.31, 0.17, 0.23), (0.05, -0.02, -4)), lookat((0.02, 0.01, 0.0), (0.0, 0.01, -4)), rng,
             t=None, p=params(sigma_world=4.0)))
    add(Case("first_call", {2}, W, H, origin, origin, rng, first_call=True))


def _size_cases(rng, add):
    for (w, h) in SIZES:
        add(Case("size_%dx%d_half_quarter" % (w, h), {1}, w, h, shifted(0.5, 0.25), camera(), rng))
        add(Case("size_%dx%d_back" % (w, h), {1}, w, h, shifted(-0.5, -0.5), camera(), rng))
        add(_motion_case("size_%dx%d_motion" % (w, h), {1, 6}, w, h, rng))


def _tap_cases(rng, add):
    origin = camera()
    for name, cam in (("", origin), ("_hxy", shifted(0.5, 0.5))):
        case = Case("divide_and_material" + name, {3}, W, H, cam, origin, rng, p=params(sigma_world=0.0, normal_cos=-1.0))
        make_miss(case.prev.features, (slice(1, 3), slice(1, 3)))
        case.prev.features[2][3:, 4:, 3] = 3.0
        case.prev.features[2][0, 6, 3] = -1.0                                                # a miss pixel's material on a hit
        add(case)
        case = Case("history_not_finite" + name, {3}, W, H, cam, origin, rng, p=params(sigma_world=0.0))
        for k, value in enumerate((np.nan, np.inf, -np.inf)):
            for word in range(4):
                y, x = divmod((k * 4 + word) * 2 + 1, W)                                     # every second pixel: each has clean neighbours
                case.prev.integrated[y, x, word] = value
        add(case)

    # dot exactly normal_cos, and one ulp below; N = (0, 0, 1)
    below = lambda x: np.nextafter(F(x), F(-np.inf))
    case = Case("normal_cos_half", {3}, W, H, origin, origin, rng, p=params(normal_cos=0.5))
    case.prev.features[1][..., :3] = (0.5, 0.5, 0.5)
    case.prev.features[1][1::2, ::2, 2] = below(0.5)
    case.prev.features[1][4, 3, :3] = np.nan
    case.pair("dot == normal_cos | one ulp below", (0, 0), (1, 0), ref.NORMAL)
    add(case)
    for cos, on, under in ((-1.0, (0, 0, -1), (0, 0, below(-1))), (0.0, (1, 0, 0), (1, 0, -1e-45)), (1.0, (0, 0, 1), (0, 0, below(1)))):
        case = Case("normal_cos_%g" % cos, {3}, W, H, origin, origin, rng, p=params(normal_cos=cos))
        case.prev.features[1][..., :3] = on
        case.prev.features[1][1::2, ::2, :3] = under
        case.pair("dot == %g | just below" % cos, (0, 0), (1, 0), ref.NORMAL)
        add(case)

    # distance exactly r * r, and the next float above: r = ( 3 * 2^-5 ) * 4 = 0.375, r * r = 9 / 64, whose ulp is 2^-26 = ( 2^-13 )^2.
    # ( 0.375^2 + ( 2^-13 )^2 ) + 0 is exact in binary32 — an ulp ON the threshold's scale, not one that rounds back onto it
    case = Case("distance_r", {3}, W, H, origin, origin, rng, p=params(sigma_world=3.0))
    case.prev.features[0][..., 0] += F(0.375)
    case.prev.features[0][1::2, ::2, 1] += F(2.0 ** -13)
    case.prev.features[0][4, 3, 2] = np.nan
    case.pair("distance == r * r | the next float above", (0, 0), (1, 0), ref.DISTANCE)
    add(case)
    case = Case("sigma_world_zero_far", {3}, W, H, origin, origin, rng, p=params(sigma_world=0.0))
    case.prev.features[0][..., :3] = 1e30
    case.prev.features[0][2, 2, :3] = np.nan
    add(case)
    case = Case("sigma_world_on_far", {3}, W, H, origin, origin, rng, p=params(sigma_world=1e-3))
    case.prev.features[0][::2, :, 1] += F(0.25)
    add(case)


def _blend_cases(rng, add):
    origin = camera()
    for mh in (1, 2, 3, 32, 1024):
        for name, cam in (("same", origin), ("hxy", shifted(0.5, 0.5))):
            case = Case("max_history_%d_%s" % (mh, name), {4}, W, H, cam, origin, rng, p=params(max_history=mh))
            ladder = np.array([1, max(mh - 1, 1), mh, 1024, 2, 1023, 31, 32, 33, min(mh + 1, 1024)], np.int64)
            case.prev.lengths[...] = ladder[(np.arange(W * H) * 3 % len(ladder))].reshape(H, W)
            case.image[1, 1, 0], case.variance[2, 2], case.image[3, 3, 3] = np.nan, np.inf, np.nan   # .w of the image is not C
            add(case)
    case = Case("input_not_finite", {4}, W, H, shifted(0.25, 0.5), origin, rng)
    for k, value in enumerate((np.nan, np.inf, -np.inf)):
        for word in range(3):
            case.image[k, word, word] = value
        case.variance[k, 4] = value
    add(case)
    case = Case("variance_zero_and_tiny_negative", {4}, W, H, shifted(0.5, 0.5), origin, rng)
    case.prev.integrated[..., 3] = 1e-3
    case.prev.integrated[::2, ::2, 3] = -1e-9
    case.prev.integrated[1::2, 1::2, 3] = 0.0
    case.variance[::3, :] = 0.0
    case.variance[1, ::2] = -1e-9
    add(case)
    case = Case("near_flt_max", {4}, W, H, shifted(0.5, 0.25), origin, rng)
    case.may_overflow[...] = True
    case.prev.integrated[...] = 3e38
    case.prev.integrated[::2, 1::2] = -3e38
    case.image[..., :3] = np.where(rng.uniform(size=(H, W, 3)) < 0.5, -3e38, 3e38)
    case.variance[...] = 3e38
    add(case)
    # tx = ty = 2^-11: bw from ( 1 - 2^-11 )^2 down to 2^-22, S = 1 exactly
    case = Case("weights_to_2^-22", {4}, W, H, shifted(2.0 ** -11, 2.0 ** -11), origin, rng)
    make_miss(case.prev.features, (slice(0, H), slice(0, W)))
    for (y, x) in ((1, 1), (2, 4), (4, 6), (3, 2)):                                          # only tap 3 of (y - 1, x - 1) is on a surface
        for plane, source in zip(case.prev.features, plane_features(camera(), PX, W, H)):
            plane[y, x] = source[y, x]
    add(case)


def _miss_cases(rng, add):
    sky_a, sky_b = lookat((0, 0, 0), (0.03, 0.05, -1), (0.1, 1, 0)), lookat((0.5, 0.5, 0.5), (0.51, 0.58, -0.5))
    case = Case("sky_to_sky_rotated", {5}, W, H, sky_a, sky_b, rng)
    make_miss(case.features, (slice(0, H), slice(0, W)))
    make_miss(case.prev.features, (slice(0, H), slice(0, W)))
    add(case)
    case = Case("sky_to_sky_65x5", {5, 1}, 65, 5, sky_b, sky_a, rng)
    make_miss(case.features, (slice(0, 5), slice(0, 65)))
    make_miss(case.prev.features, (slice(0, 5), slice(0, 65)))
    add(case)
    for name, cam in (("same", camera()), ("hxy", shifted(0.5, 0.5)), ("rotated", lookat((0.1, 0.05, 0), (0.013, 0.02, -4)))):
        case = Case("sky_beside_hits_" + name, {5}, W, H, cam, camera(), rng, t=None if name == "rotated" else DEPTH, p=params(sigma_world=4.0))
        make_miss(case.features, (slice(0, H), slice(0, 3)))
        make_miss(case.prev.features, (slice(0, 2), slice(0, W)))
        add(case)


# The motion scene: twelve faces, each on its own three vertices but face 10, which shares vertex 2 with face 0.  T0 lies in the
# plane z = -4 with e1 = ( 2, 0, 0 ), e2 = ( 0, 2, 0 ): d11 = d22 = 4, d12 = 0, den = 16 — u and v are exact.
def _motion_scene():
    a, b, c = np.array([-1, -1, -4.0]), np.array([1, -1, -4.0]), np.array([-1, 1, -4.0])
    t0 = np.stack([a, b, c])
    angle = 0.02
    turn = np.array([[np.cos(angle), -np.sin(angle), 0.01], [np.sin(angle), np.cos(angle), -0.02], [-0.01, 0.02, 1.0]])
    thin = np.stack([a, a + (2.0 ** -6, 0, 0), c])
    faces = [
        (t0, t0),                                                                    # 0 unmoved: code 1
        (t0, t0 + (1 / 16, 0, 0)),                                                   # 1 half a pixel in x, dyadic
        (t0, t0 + (0, 1 / 32, 0)),                                                   # 2 a quarter in y
        (t0, t0 @ turn.T + (0.03, 0.017, 0.002)),                                    # 3 turned
        (t0, np.stack([a, b + (0.25, 0, 0), c + (0, 0.5, 0)])),                      # 4 stretched: not rigid
        (np.stack([a, c, b]), t0 + (1 / 16, 0, 0)),                                  # 5 mirrored: dot( N, n ) < 0, n' is flipped
        (np.stack([a, c, b]), np.stack([a, c, b]) + (1 / 16, 0, 0)),                 # 6 a face seen from behind, moved rigidly
        (np.stack([a, b, b]), t0),                                                   # 7 the current face degenerate: den == 0, code 3
        (t0, np.stack([a, b, b]) + (1 / 16, 0, 0)),                                  # 8 the history's face degenerate: n' = 0, len = 0
        (thin, np.stack([(0, -1, -4.0), (3e38, -1, -4.0), (0, 1, -4.0)])),           # 9 u a multiple of 4 on e1' = 3e38: Pprev = e1' u overflows, code 3
        (None, None),                                                                # 10 shares a vertex with face 0, see below
        (t0, t0 + (1 / 16, 1 / 16, 0)),                                              # 11 the last face
    ]
    V, Hv, faces_v = [], [], []
    for k, (now, then) in enumerate(faces):
        if k == 10:
            faces_v.append((2, len(V), len(V) + 1, 0))
            V += [b, a]
            Hv += [b + (1 / 16, 0, 0), a + (1 / 16, 0, 0)]
            continue
        faces_v.append((len(V), len(V) + 1, len(V) + 2, k % 3))
        V += list(now)
        Hv += list(then)
    pad = lambda rows: np.concatenate([np.array(rows, D), np.zeros((len(rows), 1))], -1).astype(F)
    return pad(V), pad(Hv), np.array(faces_v, np.uint32)


MOTION_FACES = 12


def _motion_case(name, classes, w, h, rng, cam=None, prev_cam=None, p=None, order=None):
    # sigma_world = 0.5: r = 2^-4, and a tap half a pixel (1 / 16) away lies at exactly r * r
    case = Case(name, classes, w, h, cam or camera(), prev_cam or camera(), rng, p=p or params(sigma_world=0.5))
    V, Hv, faces_v = _motion_scene()
    order = order if order is not None else list(range(MOTION_FACES)) + [-1]
    face = np.array(order, np.int32)[np.arange(w * h) % len(order)].reshape(h, w)
    make_miss(case.features, face < 0)
    case.motion = types.SimpleNamespace(face=face, vertices=V, hist_vertices=Hv, faces_v=faces_v)
    case.may_overflow = face == 9
    return case


def _motion_cases(rng, add):
    add(_motion_case("motion_all_faces", {6}, W, H, rng))
    add(_motion_case("motion_all_faces_8x6", {6}, 8, 6, rng))
    add(_motion_case("motion_camera_moved", {6}, W, H, rng, cam=shifted(0.25, 0.25), p=params(sigma_world=2.0)))
    add(_motion_case("motion_world_term_off", {6}, W, H, rng, p=params(sigma_world=0.0, normal_cos=1.0)))
    add(_motion_case("motion_unmoved_only", {6}, W, H, rng, order=[0, -1, 0, 0]))
    # nref = ( 0, 0, 4 ) on the moved faces: N'.z = 0.5 is exactly normal_cos * len, 0.25 passes only if len is forgotten
    case = _motion_case("motion_normal_threshold", {6}, W, H, rng, order=[1, 1, 11, 0, 2])
    case.prev.features[1][..., :3] = (0, 0, 0.5)
    case.prev.features[1][1::2, :, 2] = np.nextafter(F(0.5), F(0))
    case.prev.features[1][4, :, 2] = 0.25
    case.pair("dot == normal_cos * len | one ulp below", (0, 0), (1, 1), ref.NORMAL)
    add(case)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(SEED)
    table = []
    for build in (_size_cases, _candidate_cases, _tap_cases, _blend_cases, _miss_cases, _motion_cases):
        build(rng, table.append)
    return tuple(table)


# ---- restatement and truth of a case ------------------------------------------------------------------------------------------

def restatement(case, record=None, static=ref.integrate, moving=mref.integrate):
    """-> namespace integrated, history and, on the motion path, motion, reference.  static / moving: the functions to run
    (the mutants of tests/test_temporal_planes_cpu.py come in here)."""
    feats = tuple(case.features)
    if case.motion is None:
        integrated, history = static(case.image, case.variance, feats, case.cam, case.px_dim, case.prev, case.params, record=record)
        return types.SimpleNamespace(integrated=integrated, history=history, motion=None, reference=None)
    m, planes = case.motion, {}
    integrated, history, motion = moving(case.image, case.variance, feats, m.face, m.vertices, m.hist_vertices, m.faces_v, case.cam,
                                         case.px_dim, case.prev, case.params, record=record, planes=planes)
    return types.SimpleNamespace(integrated=integrated, history=history, motion=motion, reference=planes["reference"])


@functools.lru_cache(maxsize=None)
def evaluate(case):
    """-> namespace rest, rest_record, truth, truth_record.  Treat as read-only."""
    rest_record, truth_record = ref.Record(case.h, case.w), ref.Record(case.h, case.w)
    return types.SimpleNamespace(rest=restatement(case, rest_record), rest_record=rest_record,
                                 truth=integrate_truth64(case, truth_record), truth_record=truth_record)


def device_inputs(pbr, case):
    """The arguments of Device.diag_temporal for a case."""
    def cam_of(c):
        cam = pbr.Camera()
        for k in ("eye", "u", "v", "w"):
            getattr(cam, k).x, getattr(cam, k).y, getattr(cam, k).z = (float(x) for x in c[k])
        return cam
    p = pbr.TemporalParams(int(case.params.max_history), float(case.params.normal_cos), float(case.params.sigma_world))
    prev = None
    if case.prev is not None:
        prev = dict(integrated=case.prev.integrated, features=np.stack(case.prev.features), lengths=case.prev.lengths.astype(np.uint32),
                    cam=cam_of(case.prev.cam), px_dim=float(case.prev.px_dim))
    motion = None
    if case.motion is not None:
        m = case.motion
        motion = dict(face=m.face, faces_v=m.faces_v, vertices=m.vertices, hist_vertices=m.hist_vertices)
    return dict(image=case.image, variance=case.variance, features=np.stack(case.features), cam=cam_of(case.cam), px_dim=float(case.px_dim),
                temporal=p, prev=prev, motion=motion)
