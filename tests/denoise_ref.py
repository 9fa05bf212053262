"""The a-trous filters of pbr_denoise and pbr_denoise_guided three ways, and the planted planes they are compared on.

  atrous_numpy, guided_denoise_ref.guided_numpy   the fp32 RESTATEMENTS: every operation one binary32 operation of the device
                                                  code (csrc/pt_denoise.hpp, csrc/pt_denoise_guided.hpp), in its order
  atrous_truth64, guided_truth64                  the TRUTH: the definitions in include/pbr_hip.h with every value in float64 —
                                                  exp, the sums, the two divisions, sqrt, the pass schedule

The truth takes the float32 inputs as given and keeps float64 colours and variances from pass to pass.  Two places of the
definition name binary32 and the truth follows them, because they are decisions and not values:
  * `!( e < inf )` — e is a binary32 quantity, its inf is binary32's: the truth skips a tap whose e, rounded to binary32, is
    not below inf (e >= 2^128 - 2^103, or NaN);
  * "a standard deviation of 0 switches its term off" is the term times 0: a difference that is not finite still makes e NaN
    and the tap is skipped.
The constants are the header's decimals (1e-6, 0.2126, 0.7152, 0.0722) in float64; the splines are exact in either format.

DECISIONS.  Every function can fill a list with one `Record` per pass: per pixel and tap why the tap was left out (or that it
was used), whether the pixel stayed because sum w was not in (0, inf), whether the local variance g was 0, and whether a used
weight was below 2^-126 (binary32's smallest normal: expf( -e ) is subnormal or 0 there).  tests/test_filter_planes_cpu.py
holds restatement and truth to the same decisions on every case below, and tests/test_gpu_filter_planes.py the device to the
truth's values.

CASES.  `cases()` is the one table of planted planes, seeded (SEED): see the classes in `CLASSES`."""
import types

import numpy as np

import guided_denoise_ref

F, D = np.float32, np.float64
SEED = 20
PX_DIM = F(0.01)
SMALLEST_NORMAL = 2.0 ** -126

# why a tap was left out, in the order the kernels decide
USED, OUTSIDE, DIVIDE, COLOUR, OVERFLOW, VARIANCE = 0, 1, 2, 3, 4, 5
REASONS = {USED: "used", OUTSIDE: "outside the image", DIVIDE: "across the hit / miss divide", COLOUR: "e not finite: a colour is not finite",
           OVERFLOW: "!( e < inf ) with finite colours", VARIANCE: "the tap's variance is not finite"}
CENTRE = 12          # tap (j, i) = (0, 0) in j-outer, i-inner order


class Record:
    """The decisions of one pass over an (h, w) image."""

    def __init__(self, h, w):
        self.reason = np.full((h, w, 25), 255, np.uint8)
        self.stayed = np.zeros((h, w), bool)
        self.g_zero = np.zeros((h, w), bool)
        self.tiny = np.zeros((h, w), bool)
        self.condition = np.ones((h, w))          # the truth's only: sum | w w V | / | sum w w V |, 1 without a negative variance

    def tap(self, j, i, inside, same_side, e_ok, colours_finite, variance_ok, weight):
        """What the pass did with tap (j, i) of every pixel.  e_ok: e < inf as the pass evaluated it; colours_finite: the tap's
        and the centre's colour are; variance_ok: None for the plain filter; weight: where the tap was used."""
        reason = np.full(inside.shape, USED, np.uint8)
        if variance_ok is not None:
            reason[~variance_ok] = VARIANCE
        reason[~e_ok] = np.where(colours_finite, OVERFLOW, COLOUR)[~e_ok].astype(np.uint8)
        reason[~same_side] = DIVIDE
        reason[~inside] = OUTSIDE
        self.reason[..., (j + 2) * 5 + (i + 2)] = reason
        with np.errstate(invalid="ignore"):
            self.tiny |= (reason == USED) & (np.asarray(weight, D) < SMALLEST_NORMAL)

    def only_centre(self):
        """Pixels none of whose taps but the centre lies in the image."""
        others = np.delete(self.reason, CENTRE, axis=-1)
        return (others == OUTSIDE).all(-1)

    def same_decisions(self, other):
        """(h, w) bool: tap reasons, stayed and g = 0 agree (`tiny` is a note on the weights, not a decision)."""
        return (self.reason == other.reason).all(-1) & (self.stayed == other.stayed) & (self.g_zero == other.g_zero)


def _finite3(c):
    return np.isfinite(c[..., :3]).all(-1)


def atrous_numpy(image, features, params, px_dim, record=None):
    """The definition in include/pbr_hip.h, fp32, operation for operation as csrc/pt_denoise.hpp has it.  record: a list that
    gets one Record per pass."""
    f32 = np.float32
    position, normal, albedo = features
    h, w = image.shape[:2]
    spline = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625], f32)
    cur = image.copy()
    hit = normal[..., 3] != 0

    def inverse_square(sigma):
        sigma = f32(sigma)
        return f32(1.0) / (sigma * sigma) if sigma > 0 else f32(0.0)

    def sqdist(a, b):
        d = a[..., :3] - b[..., :3]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]

    for k in range(params.passes):
        step = 1 << k
        inv_color = inverse_square(f32(params.sigma_color) / f32(1 << k))
        inv_normal, inv_albedo = inverse_square(params.sigma_normal), inverse_square(params.sigma_albedo)
        world_scale = f32(params.sigma_world) * f32(step) * f32(px_dim)
        with np.errstate(all="ignore"):
            sigma_world = world_scale * position[..., 3]
            inv_world = np.where(hit & (sigma_world > 0), f32(1.0) / (sigma_world * sigma_world), f32(0.0)).astype(f32)
        acc = np.zeros((h, w, 3), f32)
        wsum = np.zeros((h, w), f32)
        ys, xs = np.mgrid[0:h, 0:w]
        rec = Record(h, w) if record is not None else None
        for j in range(-2, 3):
            for i in range(-2, 3):
                ty, tx = ys + j * step, xs + i * step
                inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
                tyc, txc = np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)
                n, c = normal[tyc, txc], cur[tyc, txc]
                ok = inside & (n[..., 3] == normal[..., 3])
                with np.errstate(all="ignore"):
                    e = sqdist(c, cur) * inv_color
                    e_hit = e + sqdist(n, normal) * inv_normal
                    e_hit = e_hit + sqdist(position[tyc, txc], position) * inv_world
                    e_hit = e_hit + sqdist(albedo[tyc, txc], albedo) * inv_albedo
                    e = np.where(hit, e_hit, e).astype(f32)
                    ok &= e < np.inf
                    wt = np.where(ok, (spline[i + 2] * spline[j + 2]) * np.exp(-e, dtype=f32), f32(0.0)).astype(f32)
                    acc += np.where(ok[..., None], wt[..., None] * c[..., :3], f32(0.0))
                wsum += wt
                if rec is not None:
                    rec.tap(j, i, inside, n[..., 3] == normal[..., 3], e < np.inf, _finite3(c) & _finite3(cur), None, wt)
        out = cur.copy()
        usable = (wsum > 0) & np.isfinite(wsum)
        with np.errstate(all="ignore"):
            out[..., :3] = np.where(usable[..., None], acc / wsum[..., None], cur[..., :3])
        cur = out
        if rec is not None:
            rec.stayed = ~usable
            record.append(rec)
    return cur


# ---- the truth ------------------------------------------------------------------------------------------------------

SPLINE64 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625], D)
GAUSS64 = np.array([0.25, 0.5, 0.25], D)


def _inverse_square64(sigma):
    sigma = D(sigma)
    return 1.0 / (sigma * sigma) if sigma > 0 else D(0.0)


def _sqdist64(a, b):
    d = a[..., :3] - b[..., :3]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def _luminance64(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def _local_variance64(var):
    """Step 1 of the guided definition -> (g, g == 0)."""
    h, w = var.shape
    ys, xs = np.mgrid[0:h, 0:w]
    num, den = np.zeros((h, w), D), np.zeros((h, w), D)
    for j in range(-1, 2):
        for i in range(-1, 2):
            ty, tx = ys + j, xs + i
            inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
            v = var[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)]
            ok = inside & np.isfinite(v)
            g = GAUSS64[i + 1] * GAUSS64[j + 1]
            num += np.where(ok, g * np.where(ok, v, 0.0), 0.0)
            den += np.where(ok, g, 0.0)
    with np.errstate(all="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def _truth64(kind, image, var, features, params, px_dim, record):
    position, normal, albedo = (np.asarray(f, F).astype(D) for f in features)
    colour = np.asarray(image, F)[..., :3].astype(D)
    v = np.asarray(var, F).astype(D) if kind == 1 else None
    h, w = colour.shape[:2]
    hit = normal[..., 3] != 0
    ys, xs = np.mgrid[0:h, 0:w]
    first = D(F(params.sigma_color)) if kind == 0 else D(F(params.sigma_luminance))
    inv_normal, inv_albedo = _inverse_square64(F(params.sigma_normal)), _inverse_square64(F(params.sigma_albedo))

    for k in range(int(params.passes)):
        step = 1 << k
        rec = Record(h, w)
        with np.errstate(all="ignore"):
            s_world = (D(F(params.sigma_world)) * step * D(F(px_dim))) * position[..., 3]
            inv_world = np.where(hit & (s_world > 0), 1.0 / (s_world * s_world), 0.0)
            if kind == 0:
                inv_color = _inverse_square64(first / step)
            else:
                g = _local_variance64(v)
                rec.g_zero = g == 0
                scale = first * np.sqrt(g) + 1e-6
                y0 = _luminance64(colour)
        acc, wsum, vsum, vabs = np.zeros((h, w, 3), D), np.zeros((h, w), D), np.zeros((h, w), D), np.zeros((h, w), D)
        for j in range(-2, 3):
            for i in range(-2, 3):
                ty, tx = ys + j * step, xs + i * step
                inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
                tyc, txc = np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)
                n, c = normal[tyc, txc], colour[tyc, txc]
                same = n[..., 3] == normal[..., 3]
                with np.errstate(all="ignore"):
                    if kind == 0:
                        e = _sqdist64(c, colour) * inv_color
                    elif first != 0:
                        e = np.abs(_luminance64(c) - y0) / scale
                    else:
                        e = np.zeros((h, w), D)
                    e_hit = e + _sqdist64(n, normal) * inv_normal
                    e_hit = e_hit + _sqdist64(position[tyc, txc], position) * inv_world
                    e_hit = e_hit + _sqdist64(albedo[tyc, txc], albedo) * inv_albedo
                    e = np.where(hit, e_hit, e)
                    e_ok = e.astype(F) < np.inf                       # binary32's inf: see the module's docstring
                    v_ok = np.isfinite(v[tyc, txc]) if kind == 1 else None
                    ok = inside & same & e_ok & (v_ok if kind == 1 else True)
                    wt = np.where(ok, (SPLINE64[i + 2] * SPLINE64[j + 2]) * np.exp(-np.where(ok, e, 0.0)), 0.0)
                    acc += np.where(ok[..., None], wt[..., None] * c, 0.0)
                    wsum += wt
                    if kind == 1:
                        vsum += np.where(ok, (wt * wt) * v[tyc, txc], 0.0)
                        vabs += np.where(ok, np.abs((wt * wt) * v[tyc, txc]), 0.0)
                rec.tap(j, i, inside, same, e_ok, _finite3(c) & _finite3(colour), v_ok, wt)
        usable = (wsum > 0) & np.isfinite(wsum)
        rec.stayed = ~usable
        with np.errstate(all="ignore"):
            colour = np.where(usable[..., None], acc / wsum[..., None], colour)
            if kind == 1:
                v = np.where(usable, vsum / (wsum * wsum), v)
                rec.condition = np.where(usable & (vsum != 0), vabs / np.abs(np.where(vsum != 0, vsum, 1.0)), 1.0)
        if record is not None:
            record.append(rec)
    return colour, v


def atrous_truth64(image, features, params, px_dim, record=None):
    """pbr_denoise's filter as include/pbr_hip.h defines it, in float64 -> colour (H, W, 3) float64."""
    return _truth64(0, image, None, features, params, px_dim, record)[0]


def guided_truth64(image, var, features, params, px_dim, record=None):
    """pbr_denoise_guided's filter, steps 1 .. 5 of include/pbr_hip.h, in float64 -> (colour (H, W, 3), variance (H, W)) float64."""
    return _truth64(1, image, var, features, params, px_dim, record)


# ---- the planted planes ------------------------------------------------------------------------------------------------

CLASSES = {1: "hit / miss layouts the stencil straddles", 2: "colours that are not finite", 3: "variances (guided only)",
           4: "feature distances that overflow binary32", 5: "underflowing weights", 6: "standard deviations of 0",
           7: "degenerate first-hit distances", 8: "neutral"}
SIZES = ((1, 1), (1, 7), (5, 3), (8, 8), (33, 17), (70, 9), (9, 70))         # (width, height)
PASSES = (1, 3, 5, 8)
KD = np.array([[0.62, 0.58, 0.5], [0.1, 0.6, 0.2], [0.9, 0.15, 0.1]], F)    # three materials
SKY, GROUND = np.array([0.75, 0.5, 0.25], F), np.array([0.3, 0.4, 0.6], F)
DISTANCE = 4.0


def plain_params(passes=3, sigma_color=1.2, sigma_normal=0.25, sigma_world=3.0, sigma_albedo=0.1):
    return types.SimpleNamespace(passes=passes, sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_world=sigma_world, sigma_albedo=sigma_albedo)


def guided_params(passes=3, sigma_luminance=4.0, sigma_normal=0.25, sigma_world=3.0, sigma_albedo=0.1):
    return types.SimpleNamespace(passes=passes, sigma_luminance=sigma_luminance, sigma_normal=sigma_normal, sigma_world=sigma_world,
                                 sigma_albedo=sigma_albedo)


def planes(w, h, rng, hit=None, noise=0.05):
    """(image (h, w, 4), variance (h, w), features (3, h, w, 4)) float32 of a slanted wall of three materials seen from the
    origin along -z: a smooth colour plus noise, unit normals towards the viewer, positions one pixel footprint apart, the
    first-hit distance |position|; where `hit` (h, w) is False, a miss as firstHitFeatures writes it."""
    ys, xs = np.mgrid[0:h, 0:w].astype(D)
    hit = np.ones((h, w), bool) if hit is None else np.asarray(hit, bool)
    smooth = np.stack([0.5 + 0.3 * np.sin(xs / 5.0 + 0.3 * c) * np.cos(ys / 7.0 - 0.2 * c) for c in range(3)], -1)
    image = np.zeros((h, w, 4), F)
    image[..., :3] = smooth + noise * rng.normal(size=(h, w, 3))
    z = -(DISTANCE + 0.02 * xs + 0.01 * ys)
    pos = np.stack([(xs - 0.5 * w) * float(PX_DIM) * -z, (ys - 0.5 * h) * float(PX_DIM) * -z, z], -1)
    material = ((xs + 2 * ys) // 6).astype(np.int64) % 3
    lean = np.stack([0.2 * np.sin(material + 1.0), 0.1 * np.cos(material * 2.0), np.ones((h, w))], -1)
    features = np.zeros((3, h, w, 4), F)
    features[0, ..., :3], features[0, ..., 3] = pos, np.linalg.norm(pos, axis=-1)
    features[1, ..., :3], features[1, ..., 3] = lean / np.linalg.norm(lean, axis=-1, keepdims=True), 1.0
    features[2, ..., :3], features[2, ..., 3] = KD[material], material
    features[0][~hit], features[1][~hit], features[2][~hit] = [0, 0, 0, np.inf], [0, 0, 0, 0], [0, 0, 0, -1]
    image[..., 3] = features[0, ..., 3]
    variance = (noise * noise * (0.5 + rng.random((h, w)))).astype(F)
    return image, variance, features


class Case:
    """One planted input: planes, the parameters of both kinds, the classes it is there for, and the pixels (a list of (y, x))
    restatement and truth cannot decide alike on — there the expected outcome is "unchanged"."""

    def __init__(self, name, classes, w, h, image, variance, features, plain=None, guided=None, unchanged=(), kinds=(0, 1)):
        self.name, self.classes, self.w, self.h = name, frozenset(classes), w, h
        self.image, self.variance, self.features = image, variance, features
        self.params = {0: plain if plain is not None else plain_params(), 1: guided if guided is not None else guided_params()}
        self.unchanged, self.kinds = tuple(unchanged), tuple(kinds)
        for plane in (image, variance, features):
            plane.setflags(write=False)

    def __repr__(self):
        return self.name


def _layout(kind, period, w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    if kind == "stripes":
        return (xs // period) % 2 == 0
    return ((xs // period) + (ys // period)) % 2 == 0


def _build():
    out = []

    def add(name, classes, w, h, image, variance, features, **more):
        out.append(Case(name, classes, w, h, np.ascontiguousarray(image, F), np.ascontiguousarray(variance, F), np.ascontiguousarray(features, F), **more))

    def rng_of(name):
        return np.random.default_rng([SEED] + [ord(ch) for ch in name])

    # 8. a random hit plane with no edge at all, every size and pass count
    for (w, h) in SIZES:
        for passes in PASSES:
            name = "neutral_%dx%d_p%d" % (w, h, passes)
            add(name, {8}, w, h, *planes(w, h, rng_of("neutral_%dx%d" % (w, h))), plain=plain_params(passes), guided=guided_params(passes))

    # 1. stripes and checkerboards of hit and miss, constant colours on either side; single pixels
    for (w, h) in ((33, 17), (70, 9), (9, 70)):
        for kind in ("stripes", "checker"):
            for period in (1, 2, 4, 16):
                for passes in (1, 3, 8):
                    name = "%s%d_%dx%d_p%d" % (kind, period, w, h, passes)
                    hit = _layout(kind, period, w, h)
                    image, variance, features = planes(w, h, rng_of(name), hit)
                    image[..., :3] = np.where(hit[..., None], GROUND, SKY)
                    add(name, {1}, w, h, image, variance, features, plain=plain_params(passes), guided=guided_params(passes))
    for what in ("hit_in_sky", "sky_in_geometry"):
        for passes in (1, 3):
            w, h = 33, 17
            hit = np.full((h, w), what == "sky_in_geometry")
            hit[8, 16] = not hit[8, 16]
            name = "%s_p%d" % (what, passes)
            image, variance, features = planes(w, h, rng_of(name), hit)
            image[..., :3] = np.where(hit[..., None], GROUND, SKY)
            add(name, {1}, w, h, image, variance, features, plain=plain_params(passes), guided=guided_params(passes))

    # 2. NaN, +Inf, -Inf: as a centre (each planted pixel is one), as an inner and an outer tap (of its neighbours), in the corners;
    # one channel only; a whole row of NaN.  Half the image is sky, so both classes of centre meet them.
    for passes in (1, 3, 8):
        w, h = 33, 17
        name = "nonfinite_colour_p%d" % passes
        hit = np.mgrid[0:h, 0:w][1] >= 10
        image, variance, features = planes(w, h, rng_of(name), hit)
        image[5, 5, :3], image[8, 12, :3], image[11, 20, :3] = np.nan, np.inf, -np.inf
        image[5, 25, 1], image[3, 3, 2], image[3, 18, 0] = np.nan, np.inf, -np.inf
        image[0, 0, :3], image[0, w - 1, :3], image[h - 1, 0, :3], image[h - 1, w - 1, :3] = np.nan, np.inf, -np.inf, np.nan
        image[14, :, :3] = np.nan
        add(name, {2}, w, h, image, variance, features, plain=plain_params(passes), guided=guided_params(passes))
    # the guided filter's luminance term off: e_l = 0 whatever the colours are, so a tap that is not finite is NOT left out (step 2)
    name = "nonfinite_colour_luminance_off"
    image, variance, features = planes(33, 17, rng_of(name))
    image[5, 5, :3], image[8, 12, :3], image[11, 20, 1] = np.nan, np.inf, -np.inf
    add(name, {2, 6}, 33, 17, image, variance, features, guided=guided_params(2, sigma_luminance=0.0), kinds=(1,))

    # 3. variances: one pixel, a 3 x 3 neighbourhood, the whole image.  Grey colours in steps of 1 / 64, so that where g = 0 makes
    # the scale 1e-6 a tap's e is 0 or > 1e4: its weight is 0 in either format and the decisions cannot part.
    def grey(image):
        image[..., :3] = np.round(image[..., 1:2] * 64.0) / 64.0
        return image
    # A negative variance is finite: it takes part.  Next to positive ones sum w w V can cancel to any degree, and an error
    # relative to |truth| then measures the cancellation, not the filter — so in one pixel and in a block it is -1e-9 against
    # neighbours of 1e-3 (sum | w w V | / | sum w w V | stays below 1.001, which tests/test_filter_planes_cpu.py holds on the truth
    # for every case); the whole image is -1, where every g is negative, sd = NaN and every pixel stays.
    for what, value in (("nan", np.nan), ("inf", np.inf), ("zero", 0.0), ("negative", -1.0)):
        for extent in ("pixel", "block", "all"):
            for passes in (1, 3):
                w, h = 33, 17
                name = "variance_%s_%s_p%d" % (what, extent, passes)
                planted = -1e-9 if what == "negative" and extent != "all" else value
                image, variance, features = planes(w, h, rng_of(name), np.mgrid[0:h, 0:w][1] >= 6)
                image = grey(image)
                if extent == "pixel":
                    variance[8, 16], variance[8, 2] = planted, planted
                elif extent == "block":
                    variance[7:10, 15:18], variance[0:2, 0:2], variance[7:10, 1:4] = planted, planted, planted
                    # one grey around each block: taps of the same material keep weights far above binary32's underflow, so
                    # that sum w * sum w does not vanish in one format only
                    image[5:12, 13:20, :3], image[0:4, 0:4, :3], image[5:12, 0:6, :3] = 0.40625, 0.40625, 0.40625
                else:
                    variance[...] = planted
                add(name, {3}, w, h, image, variance, features, guided=guided_params(passes), kinds=(1,))

    # 4. positions 1e20 apart (their squared distance overflows binary32, sigma_world small enough that the truth's e does too up
    # to 8 passes); colours 1e19 apart with a small sigma_color (guided: the luminance step's e is finite and its weight 0)
    for passes in (1, 3, 8):
        w, h = 33, 17
        name = "far_positions_p%d" % passes
        image, variance, features = planes(w, h, rng_of(name))
        for (y, x) in ((8, 16), (2, 30), (15, 0), (9, 16)):
            features[0, y, x, 0] += 1e20
        add(name, {4}, w, h, image, variance, features, plain=plain_params(passes, sigma_world=0.5), guided=guided_params(passes, sigma_world=0.5))
        name = "far_colours_p%d" % passes
        image, variance, features = planes(w, h, rng_of(name), np.mgrid[0:h, 0:w][1] >= 12)
        image[8, 16, :3], image[8, 4, :3], image[3, 20, :3], image[0, 0, :3] = 1e19, -1e19, [1e19, 0.5, -1e19], 1e19
        add(name, {4}, w, h, image, variance, features, plain=plain_params(passes, sigma_color=0.1), guided=guided_params(passes))

    # 5. e across 80 .. 110 on a featureless wall: lone pixels that much above a constant grey, five pixels apart.  Plain:
    # e = 3 d^2 / sigma_color^2.  Guided: e = d ( 0.2126 + 0.7152 + 0.0722 ) / ( sigma_luminance sqrt( v ) + 1e-6 ), v constant.
    for passes in (1, 3):
        w, h = 70, 9
        name = "underflow_p%d" % passes
        image, variance, features = planes(w, h, rng_of(name), noise=0.0)
        features[1, ..., :3], features[2, ..., :3], features[2, ..., 3] = [0, 0, 1], KD[0], 0
        targets = np.linspace(80.0, 110.0, 26)
        spots = [(2 + 5 * (n // 13), 3 + 5 * (n % 13)) for n in range(26)]
        for kind in (0, 1):
            img, var = image.copy(), np.full((h, w), 0.0025, F)
            img[..., :3] = 0.25
            for (y, x), e in zip(spots, targets):
                img[y, x, :3] = 0.25 + (np.sqrt(e / 3.0) * 0.5 if kind == 0 else e * (2.0 * 0.05 + 1e-6))
            add("%s_%s" % (name, ("plain", "guided")[kind]), {5}, w, h, img, var, features.copy(),
                plain=plain_params(passes, sigma_color=0.5, sigma_normal=0.0, sigma_world=0.0, sigma_albedo=0.0),
                guided=guided_params(passes, sigma_luminance=2.0, sigma_normal=0.0, sigma_world=0.0, sigma_albedo=0.0), kinds=(kind,))

    # 6. every standard deviation 0 on its own, and all: the pure B3 spline — also on a constant image
    for off in ("first", "sigma_normal", "sigma_world", "sigma_albedo", "all"):
        w, h = 33, 17
        name = "off_%s" % off
        image, variance, features = planes(w, h, rng_of(name), _layout("stripes", 16, w, h))
        zero = {"first": ("sigma_color", "sigma_luminance"), "all": None}.get(off, (off, off))
        p = {k: 0.0 for k in ("sigma_color", "sigma_normal", "sigma_world", "sigma_albedo")} if zero is None else {zero[0]: 0.0}
        g = {k: 0.0 for k in ("sigma_luminance", "sigma_normal", "sigma_world", "sigma_albedo")} if zero is None else {zero[1]: 0.0}
        add(name, {6}, w, h, image, variance, features, plain=plain_params(3, **p), guided=guided_params(3, **g))
    for (w, h) in ((33, 17), (70, 9)):
        name = "off_all_constant_%dx%d" % (w, h)
        image, variance, features = planes(w, h, rng_of(name))
        image[..., :3] = [0.3, 0.7, 0.1]
        add(name, {6}, w, h, image, variance, features, plain=plain_params(5, 0.0, 0.0, 0.0, 0.0), guided=guided_params(5, 0.0, 0.0, 0.0, 0.0))

    # 7. first-hit distance 0 (invWorld = 0: the term is off), subnormal and 1e-30 (sigmaWorld^2 underflows in binary32 only:
    # invWorld = inf, e = NaN at the centre, the pixel stays — in float64 every other tap's weight is 0 and the centre's colour
    # comes back), 1e30 (sigmaWorld^2 overflows: invWorld = 0)
    for passes in (1, 3, 8):
        w, h = 33, 17
        name = "degenerate_distance_p%d" % passes
        image, variance, features = planes(w, h, rng_of(name))
        spots = {(3, 4): 0.0, (3, 12): 1e-40, (8, 16): 1e-30, (12, 25): 1e30, (0, 0): 1e-30, (16, 32): 1e-40}
        for (y, x), t in spots.items():
            features[0, y, x, 3] = t
        add(name, {7}, w, h, image, variance, features, plain=plain_params(passes), guided=guided_params(passes),
            unchanged=[at for at, t in spots.items() if 0 < t < 1e-20])
    return out


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = _build()
    return _cases


# ---- restatement against truth, once per (case, kind) ----------------------------------------------------------------------

_evaluated = {}


def evaluate(case, kind):
    """types.SimpleNamespace of a case under one kind: rest (rgba, variance | None) and rest_record of the fp32 restatement;
    truth (colour64, variance64 | None) and truth_record; e_ref, the largest |restatement - truth| over the colour channels the
    truth has finite; e_ref_variance, the same relative to |truth| over its finite, non-zero variances (None for kind 0)."""
    key = (case.name, kind)
    if key not in _evaluated:
        p, feats = case.params[kind], tuple(case.features)
        r = types.SimpleNamespace(rest_record=[], truth_record=[], e_ref_variance=None)
        if kind == 0:
            r.rest = (atrous_numpy(case.image, feats, p, PX_DIM, r.rest_record), None)
            r.truth = (atrous_truth64(case.image, feats, p, PX_DIM, r.truth_record), None)
        else:
            r.rest = guided_denoise_ref.guided_numpy(case.image, case.variance, feats, p, PX_DIM, record=r.rest_record)
            r.truth = guided_truth64(case.image, case.variance, feats, p, PX_DIM, r.truth_record)
            r.e_ref_variance = relative_error(r.rest[1], r.truth[1])
        r.e_ref = colour_error(r.rest[0], r.truth[0])
        _evaluated[key] = r
    return _evaluated[key]


def colour_error(got, truth):
    """max |got - truth| over the colour channels that are finite in the truth (0 if none is)."""
    finite = np.isfinite(truth)
    with np.errstate(invalid="ignore"):
        diff = np.abs(np.asarray(got, D)[..., :3] - truth)[finite]
    return float(diff.max()) if diff.size else 0.0


def relative_error(got, truth):
    """max |got - truth| / |truth| over the finite, non-zero values of the truth (0 if there is none)."""
    use = np.isfinite(truth) & (truth != 0)
    with np.errstate(invalid="ignore"):
        diff = (np.abs(np.asarray(got, D) - truth) / np.abs(np.where(use, truth, 1.0)))[use]
    return float(diff.max()) if diff.size else 0.0


def largest_colour(case):
    c = np.abs(case.image[..., :3].astype(D))
    c = c[np.isfinite(c)]
    return float(c.max()) if c.size else 0.0


def ulp32(x):
    """One binary32 unit in the last place of |x|."""
    return float(np.spacing(F(abs(x))))


# ---- a result against the truth: what tests/test_gpu_filter_planes.py asks of the device ---------------------------------------

def _same_bits(a, b):
    return np.ascontiguousarray(a, F).view(np.uint32) == np.ascontiguousarray(b, F).view(np.uint32)


def against_truth(case, kind, rgba, variance=None):
    """A filter's output on a case held to the truth -> (failures: a list of sentences, empty if it passes; the largest colour
    error; the largest relative variance error, None for kind 0).
    Exact: .w is the image's; the values that are not finite are the truth's; a pixel the truth leaves as it was in every pass, and
    a pixel of case.unchanged, has its input's bits; where the truth's variance is 0, so is this one.
    Toleranced: colours within 4 E_ref + one binary32 ulp of the case's largest finite colour, variances within 4 E_ref + 2^-23
    relative — E_ref is the restatement's distance from the truth on this case (`evaluate`)."""
    r = evaluate(case, kind)
    rgba = np.asarray(rgba, F)
    truth_colour, truth_variance = r.truth
    failures = []
    if not _same_bits(rgba[..., 3], case.image[..., 3]).all():
        failures.append(".w is not the image's .w")
    if not (np.isfinite(rgba[..., :3]) == np.isfinite(truth_colour)).all():
        failures.append("the colours that are not finite are not the truth's: %d values differ" % (np.isfinite(rgba[..., :3]) != np.isfinite(truth_colour)).sum())
    stayed = np.logical_and.reduce([rec.stayed for rec in r.truth_record])
    for (y, x) in case.unchanged:
        stayed[y, x] = True
    if not _same_bits(rgba[..., :3], case.image[..., :3])[stayed].all():
        failures.append("a pixel that stays has not kept its colour's bits")
    colour = colour_error(rgba, truth_colour)
    bound = 4.0 * r.e_ref + ulp32(largest_colour(case))
    if not colour <= bound:
        failures.append("colour error %.3e > 4 * %.3e + %.3e" % (colour, r.e_ref, ulp32(largest_colour(case))))
    relative = None
    if kind == 1:
        variance = np.asarray(variance, F)
        if not (np.isfinite(variance) == np.isfinite(truth_variance)).all():
            failures.append("the variances that are not finite are not the truth's: %d values differ" % (np.isfinite(variance) != np.isfinite(truth_variance)).sum())
        if not _same_bits(variance, case.variance)[stayed].all():
            failures.append("a pixel that stays has not kept its variance's bits")
        if not (variance[truth_variance == 0] == 0).all():
            failures.append("a variance is not 0 where the truth's is")
        relative = relative_error(variance, truth_variance)
        if not relative <= 4.0 * r.e_ref_variance + 2.0 ** -23:
            failures.append("relative variance error %.3e > 4 * %.3e + 2^-23" % (relative, r.e_ref_variance))
    return failures, colour, relative
