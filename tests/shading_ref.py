"""A float64 restatement of the shading stages: BRDF evaluation, new-ray sampling, and what a bounce does with them
(updateColor and the composed surface step).

The oracle (oracle/pt_oracle.c) and the HIP kernels are checked against each other bit for bit; this module is the
independent check of both.  It is derived from the reference's OpenCL sources, not from either implementation:

  source/opencl/pt_brdf.cl   Z, A, G, B2, D (11-112), brdfSchlick (125-149), newRaySchlick (159-208),
                             brdfShirleyAshikhmin (228-268), newRayShirleyAshikhmin (278-330), getNewRay (344-378)
  source/opencl/pt_utils.cl  bisect (7), rand (39-44), fresnel (53-56), jitter (306-318), reflect (426),
                             refract (436-465)
  source/opencl/pt_header.cl NI_AIR (13), PI_X2 (17)
  source/opencl/pathtracing.cl updateColor (89-178), and the lines of the kernel around it (281-303): getNewRay from the
                             unflipped normal, the normal flip, updateColor

Everything is numpy float64, vectorised over samples.  The reference's quirks are kept: the Schlick pdf is
t / ( 4 pi dot( V_OUT, h ) ) as written, the tangent frame is cross( n.yzx, n ) (undefined for a normal along
+-(1,1,1)), a translucent material (d < 1) never flips its normal in the Shirley-Ashikhmin sampler.

Three things are NOT computed here, by design:

  * Random numbers.  The reference's rand is a float32 hash, fract( sin( seed ) * 43758.5453 ) with seed += 1 per draw;
    one ulp changes it completely.  The seed sequence s_j = fl32( s_(j-1) + 1 ) is formed here (`seed_sequence`) and the
    draws come from the arithmetic under test; they are inputs.  The reference predicts how many a sample takes.
  * Branch decisions on computed quantities (sinT2 >= 1, reflectance < rnd, dot( spec, n ) <= 0, into, dotHN == 1, the
    x == 0 guards of Z / A / G, ...).  They are decided in float64; where the quantity lies within its own error bound
    of the threshold the sample is AMBIGUOUS and the result of either branch is accepted (`check`).  Decisions on inputs
    alone (a material value against a constant, a draw against 0.25) are exact.
  * Tolerances by hand.  Per sample and output the reference's own sensitivity Delta is measured by finite differences
    (`Analysis`): every input, draws included, moved by one float32 ulp either way, and a few evaluations in which every
    rounding point of the float32 computation (`_Ev.r`: each statement of the reference and the terms of each
    cancelling difference) is moved by a relative 2^-24 of random sign; the branches are held to the unperturbed ones.
    A result passes when |got - ref| <= K * ( 2^-24 * |ref| + Delta + 2^-149 ); direction components use 1 in place of
    |ref|.
    Where the reference is non-finite (and stays so under every perturbation) the result must be non-finite too.
"""
import numpy as np

U = 2.0 ** -24                               # unit roundoff of binary32
NI_AIR = float(np.float32(1.00028))          # pt_header.cl:13, a float literal
PI_X2 = float(np.float32(6.28318530718))     # pt_header.cl:17, a float literal
PD_SCALE = float(np.float32(0.38750768752))  # pt_brdf.cl:256, a float literal
PI = np.pi                                   # M_PI, M_PI_2, M_1_PI: double literals, the expressions are double
TINY = 2.0 ** -149                           # the smallest binary32 step: a result below the format's range is 0
DRAWS = 4                                    # the most draws one getNewRay sample takes: the d test, a, b, the fallback


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def seed_sequence(seed, k=DRAWS):
    """(n, k + 1) float32: s_0 = seed, s_j = fl32( s_(j-1) + 1 ) (pt_utils.cl:41)."""
    s = [np.asarray(seed, np.float32)]
    for _ in range(k):
        s.append((s[-1] + np.float32(1.0)).astype(np.float32))
    return np.stack(s, axis=-1)


# ---------------------------------------------------------------------------------------------------------------------
# one evaluation: rounding points and decisions
# ---------------------------------------------------------------------------------------------------------------------

class _Ev:
    """State of one vectorised evaluation.  force: decisions to take from another evaluation instead of computing them;
    rng: when given, every rounding point is moved by a relative 2^-24 of random sign (2^-150 absolute for a subnormal)."""

    def __init__(self, n, force=None, rng=None, flush=False):
        self.n, self.force, self.rng, self.flush = n, force or {}, rng, flush
        self.dec, self.q = {}, {}

    def r(self, x):
        # a rounding point is a binary32 value: below half the smallest subnormal it IS zero and past the largest finite
        # value it IS infinite, with whatever follows from that (the quotient of two such values is 0 / 0 or inf / inf, not
        # their ratio)
        with np.errstate(invalid="ignore"):
            x = np.where(np.abs(x) < 2.0 ** -150, np.copysign(0.0, x), x)
            x = np.where(np.abs(x) >= 2.0 ** 128 * (1.0 - 2.0 ** -25), np.copysign(np.inf, x), x)
        if self.rng is None:
            return x
        sign = self.rng.choice((-1.0, 1.0), size=np.shape(x))
        # below the normal range binary32 rounds to a multiple of 2^-149: half of that, absolute; an arithmetic that
        # flushes subnormal results (flush) makes them 0
        tiny = 0.0 if self.flush else x + sign * 2.0 ** -150
        return np.where((x != 0) & (np.abs(x) < 2.0 ** -126), tiny, x * (1.0 + U * sign))

    def decide(self, key, cond, q=None, scale=1.0, active=None):
        """A branch.  q: the computed quantity minus its threshold (None: an exact decision on inputs); scale: what the
        quantity's rounding is relative to; active: the samples that reach the branch.  A decision held from another
        evaluation is recomputed where that evaluation had no quantity to decide on (q NaN)."""
        cond = np.broadcast_to(np.asarray(cond, bool), (self.n,))
        act = np.ones(self.n, bool) if active is None else active
        free = act & np.isnan(q) if q is not None else np.zeros(self.n, bool)
        if key in self.force:
            held, was_free = self.force[key]
            cond = np.where(was_free, cond, held)
            free = free & was_free
        self.dec[key] = (cond, free)
        if q is not None:
            self.q[key] = (np.where(act, q, np.inf), np.where(act, np.abs(scale), 0.0))
        return cond


def _dot(ev, a, b):
    return ev.r(np.einsum("ij,ij->i", a, b))


def _cross(ev, a, b):
    return ev.r(np.cross(a, b))


def _yzx(a):
    return a[:, [1, 2, 0]]


def _normalize(ev, a):
    """fast_normalize: a * ( 1 / sqrt( dot( a, a ) ) ); the zero vector gives NaN, as 0 * ( 1 / sqrt( 0 ) ) does.  The
    rounding of the common factor moves every component the same way."""
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = ev.r(1.0 / ev.r(np.sqrt(_dot(ev, a, a))))
        return ev.r(a * inv[:, None])


def _reflect(ev, d, n):
    """pt_utils.cl:426: dir - 2 dot( normal, dir ) normal."""
    return ev.r(d - 2.0 * _dot(ev, n, d)[:, None] * n)


def _jitter(ev, nl, phi, sina, cosa):
    """pt_utils.cl:306-318."""
    u = _normalize(ev, _cross(ev, _yzx(nl), nl))
    v = _normalize(ev, _cross(ev, nl, u))
    c, s = ev.r(np.cos(phi)), ev.r(np.sin(phi))
    t = _normalize(ev, ev.r(u * c[:, None] + v * s[:, None]))
    return _normalize(ev, ev.r(t * sina[:, None] + nl * cosa[:, None]))


def _fresnel(ev, u, c):
    """pt_utils.cl:53-56: c + ( 1 - c ) ( 1 - u )^5."""
    v = ev.r(1.0 - u)
    return ev.r(c + ev.r(ev.r(1.0 - c) * ev.r(v ** 5)))


def _acos(x):
    """acos of a quantity that is in [-1, 1] in exact arithmetic: a rounding (or a perturbation) just outside is not
    a NaN of the reference's."""
    return np.arccos(np.clip(x, -1.0, 1.0))


def _sqrt(x):
    """sqrt of a quantity that is >= 0 in exact arithmetic."""
    return np.sqrt(np.maximum(x, 0.0))


def _sel(cond, a, b):
    return np.where(cond[:, None] if np.ndim(a) == 2 or np.ndim(b) == 2 else cond, a, b)


def _pow(ev, key, x, y, active):
    """pow( x, y ), C99.  A negative base has a real power only at an integer exponent; whether a computed exponent IS
    an integer is a decision on a computed quantity, ambiguous within the exponent's own error bound."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        neg = x < 0
        yr = np.rint(y)
        # a float of magnitude 2^24 or more is an integer
        is_int = ev.decide(key, (np.abs(y) >= 2.0 ** 24) | (y == yr), q=np.where(neg, y - yr, np.inf), scale=y, active=active & neg)
        mag = np.abs(x) ** np.where(is_int, yr, y)
        odd = is_int & (np.mod(yr, 2) == 1)
        neg_val = np.where(is_int, np.where(odd, -mag, mag), np.nan)
        return np.where(neg, neg_val, np.power(np.where(neg, 1.0, x), y))


# ---------------------------------------------------------------------------------------------------------------------
# Schlick (BRDF 0): material data = d, Ni, p, rough
# ---------------------------------------------------------------------------------------------------------------------

def _Z(ev, key, t, r, active):
    """pt_brdf.cl:11-14."""
    tt = ev.r(t * t)
    x = ev.r(ev.r(1.0 + ev.r(r * tt)) - tt)
    zero = ev.decide(key, x == 0.0, q=x, scale=1.0 + tt, active=active)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(zero, 0.0, ev.r(r / ev.r(x * x)))


def _A(ev, key, w, p, active):
    """pt_brdf.cl:23-28."""
    p2, w2 = ev.r(p * p), ev.r(w * w)
    x = ev.r(ev.r(p2 - ev.r(p2 * w2)) + w2)
    zero = ev.decide(key, x == 0.0, q=x, scale=p2 + w2, active=active)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(zero, 0.0, ev.r(np.sqrt(ev.r(p / x))))


def _G(ev, key, v, r, active):
    """pt_brdf.cl:37-40."""
    x = ev.r(ev.r(r - ev.r(r * v)) + v)
    zero = ev.decide(key, x == 0.0, q=x, scale=np.abs(r) + np.abs(v), active=active)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(zero, 0.0, ev.r(v / x))


def _D(ev, t, vOut, vIn, w, r, p):
    """pt_brdf.cl:93-112, with B2 (71-80)."""
    on = np.ones(ev.n, bool)
    b = ev.r(4.0 * r * ev.r(1.0 - r))
    low = ev.decide("D.low", r < 0.5)
    a = np.where(low, 0.0, ev.r(1.0 - b))
    c = np.where(low, ev.r(1.0 - b), 0.0)
    d = ev.r(ev.r(4.0 * PI * vOut) * vIn)
    lam = ev.r(a / PI)
    b0 = ev.decide("D.b0", (r == 0.0) | (r == 1.0))     # 4 r ( 1 - r ) == 0: exactly at the inputs r = 0 and r = 1
    vout0 = ev.decide("D.vOut0", vOut == 0.0, q=vOut, active=~b0)
    vin0 = ev.decide("D.vIn0", vIn == 0.0, q=vIn, active=on)
    ani_on = ~(b0 | vout0 | vin0)
    gp = ev.r(_G(ev, "G.out0", vOut, r, ani_on) * _G(ev, "G.in0", vIn, r, ani_on))
    obstructed = ev.r(ev.r(gp * _Z(ev, "Z0", t, r, ani_on)) * _A(ev, "A0", w, p, ani_on))
    B2 = ev.r(obstructed + ev.r(1.0 - gp))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ani = np.where(ani_on, ev.r(ev.r(b / d) * B2), 0.0)
        fres = np.where(vin0, 0.0, ev.r(c / vIn))
    return ev.r(ev.r(lam + ani) + fres)


def _half_vector(ev, v_out, v_in):
    """h = fast_normalize( V_OUT + V_IN ).  In the surface step's evaluation at the SAMPLED direction (an evaluation that
    says so: `opposite_undefined`, set by surface_step alone) the two directions can be opposite — a ray transmitted
    straight through, a mirror hit at exactly grazing incidence —, the sum is zero or its own rounding noise in binary32
    and h is 0 / 0 or noise: undefined in the reference itself.  Such a sample is NaN there and finite noise under the
    rounding trials, so that its measured sensitivity is infinite and `judge` accepts whatever the arithmetic under test
    makes of it.  Everywhere else this is the plain normalisation."""
    s = ev.r(v_out + v_in)
    if getattr(ev, "opposite_undefined", False) and ev.rng is None:
        gone = (s * s).sum(axis=1) <= (16.0 * U) ** 2
        s = np.where(gone[:, None], np.nan, s)
    return _normalize(ev, s)


def brdf_schlick(ev, mtl, x):
    """pt_brdf.cl:125-149 -> (n, 3) {brdf, u, pdf}."""
    p, r = mtl[2], mtl[3]
    normal, v_in, v_out = x["normal"], x["in"], -x["out"]
    un = _normalize(ev, _cross(ev, _yzx(normal), normal))
    h = _half_vector(ev, v_out, v_in)
    t = _dot(ev, h, normal)
    vIn = _dot(ev, v_in, normal)
    vOut = _dot(ev, v_out, normal)
    hp = _normalize(ev, _cross(ev, _cross(ev, h, normal), normal))
    w = _dot(ev, un, hp)
    u = _dot(ev, h, v_out)
    with np.errstate(divide="ignore", invalid="ignore"):
        pdf = ev.r(t / ev.r(4.0 * PI * _dot(ev, v_out, h)))
    brdf = _D(ev, t, vOut, vIn, w, r, p)
    return {"val": np.stack([brdf, u, pdf], axis=1)}


def _new_ray_schlick(ev, mtl, d, n, draw, active):
    """pt_brdf.cl:159-208 -> (direction, draws taken)."""
    p, r = mtl[2], mtl[3]
    mirror = ev.decide("S.mirror", r == 0.0)
    go = active & ~mirror
    a, b = draw(0), draw(1)
    iso2 = ev.r(p * p)
    quad = np.select([ev.decide("S.b0", b < 0.25), ev.decide("S.b1", b < 0.5), ev.decide("S.b2", b < 0.75)], [0, 1, 2], 3)
    top = np.choose(quad, [0.25, 0.5, 0.75, 1.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = ev.r(_acos(ev.r(_sqrt(ev.r(a / ev.r(ev.r(r - ev.r(a * r)) + a))))))
        bb = ev.r(1.0 - ev.r(4.0 * ev.r(top - b)))
        b2 = ev.r(bb * bb)
        phi0 = ev.r(PI / 2 * ev.r(_sqrt(ev.r(ev.r(iso2 * b2) / ev.r(ev.r(1.0 - b2) + ev.r(b2 * iso2))))))
    phi = np.choose(quad, [phi0, ev.r(PI - phi0), ev.r(PI + phi0), ev.r(2.0 * PI - phi0)])
    phi = np.where(ev.decide("S.aniso", p < 1.0), ev.r(phi + PI / 2), phi)
    H = _jitter(ev, n, phi, ev.r(np.sin(alpha)), ev.r(np.cos(alpha)))
    ray = _reflect(ev, d, H)
    dn = _dot(ev, ray, n)
    below = ev.decide("S.below", dn <= 0.0, q=dn, active=go)
    with np.errstate(invalid="ignore"):
        diff = _jitter(ev, n, ev.r(PI_X2 * draw(2)), ev.r(_sqrt(a)), ev.r(_sqrt(ev.r(1.0 - a))))
    ray = _sel(below, diff, ray)
    return _sel(mirror, _reflect(ev, d, n), ray), np.where(mirror, 0, np.where(below, 3, 2))


# ---------------------------------------------------------------------------------------------------------------------
# Shirley-Ashikhmin (BRDF 1): material data = d, Ni, nu, nv, Rs, Rd
# ---------------------------------------------------------------------------------------------------------------------

def brdf_shirley_ashikhmin(ev, mtl, x):
    """pt_brdf.cl:228-268 -> (n, 4) {spec, diff, dotHK1, pdf}."""
    nu, nv, Rd = mtl[2], mtl[3], mtl[5]
    normal = x["normal"]
    on = np.ones(ev.n, bool)
    un = _normalize(ev, _cross(ev, _yzx(normal), normal))
    vn = _normalize(ev, _cross(ev, normal, un))
    k1, k2 = x["in"], -x["out"]
    h = _half_vector(ev, k2, k1)
    dotHU, dotHV, dotHN = _dot(ev, h, un), _dot(ev, h, vn), _dot(ev, h, normal)
    dotNK1, dotNK2 = _dot(ev, normal, k1), _dot(ev, normal, k2)
    dotHK1 = _dot(ev, h, k1)
    ps_e = ev.r(ev.r(nu * ev.r(dotHU * dotHU)) + ev.r(nv * ev.r(dotHV * dotHV)))
    hn1 = ev.decide("SA.hn1", dotHN == 1.0, q=dotHN - 1.0, active=on)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ps_e = np.where(hn1, 0.0, ev.r(ps_e / ev.r(1.0 - ev.r(dotHN * dotHN))))
        ps0 = ev.r(ev.r(ev.r(np.sqrt(ev.r((nu + 1.0) * (nv + 1.0)))) * 0.125) / PI)
        ps1_num = ev.r(_pow(ev, "SA.pow", dotHN, ps_e, on))
        ps1 = ev.r(ps1_num / ev.r(dotHK1 * np.maximum(dotNK1, dotNK2)))
        pd = ev.r(Rd * PD_SCALE)
        a = ev.r(1.0 - ev.r(dotNK1 * 0.5))
        b = ev.r(1.0 - ev.r(dotNK2 * 0.5))
        pd = ev.r(pd * ev.r(1.0 - ev.r(a ** 5)))
        pd = ev.r(pd * ev.r(1.0 - ev.r(b ** 5)))
        spec = ev.r(ps0 * ps1)
        pdf = ev.r(ev.r(ps0 * ps1_num) / dotHK1)
    return {"val": np.stack([spec, pd, dotHK1, pdf], axis=1)}


def _new_ray_shirley_ashikhmin(ev, mtl, d, n, draw, active):
    """pt_brdf.cl:278-330 -> (direction, draws taken)."""
    dd, nu, nv = mtl[0], mtl[2], mtl[3]
    a, b = draw(0), draw(1)
    quad = np.select([ev.decide("SA.a0", a < 0.25), ev.decide("SA.a1", a < 0.5), ev.decide("SA.a2", a < 0.75)], [0, 1, 2], 3)
    a_max = np.choose(quad, [0.25, 0.5, 0.75, 1.0])
    phi_flip = np.choose(quad, [0.0, f32(PI), f32(PI), f32(2.0 * PI)])     # `float phi_flip = M_PI`: stored as a float
    phi_flipf = np.choose(quad, [1.0, -1.0, 1.0, -1.0])
    a = ev.r(1.0 - ev.r(4.0 * ev.r(a_max - a)))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        phi = ev.r(np.arctan(ev.r(ev.r(np.sqrt(ev.r((nu + 1.0) / (nv + 1.0)))) * ev.r(np.tan(ev.r(PI / 2 * a))))))
        phi_full = ev.r(phi_flip + ev.r(phi_flipf * phi))
        cosphi, sinphi = ev.r(np.cos(phi)), ev.r(np.sin(phi))
        theta_e = ev.r(1.0 / ev.r(ev.r(ev.r(ev.r(nu * cosphi) * cosphi) + ev.r(ev.r(nv * sinphi) * sinphi)) + 1.0))
        theta = ev.r(_acos(ev.r(np.power(ev.r(1.0 - b), theta_e))))
    front = _dot(ev, n, -d)
    solid = ev.decide("SA.solid", dd >= 1.0)
    keep = ev.decide("SA.front", front >= 0.0, q=front, active=active & solid)
    normal = _sel(~solid | keep, n, -n)
    h = _jitter(ev, normal, phi_full, ev.r(np.sin(theta)), ev.r(np.cos(theta)))
    spec = _reflect(ev, d, h)
    with np.errstate(invalid="ignore"):
        diff = _jitter(ev, normal, ev.r(PI_X2 * draw(2)), ev.r(_sqrt(b)), ev.r(_sqrt(ev.r(1.0 - b))))
    sn = _dot(ev, spec, normal)
    use_diff = ev.decide("SA.below", sn <= 0.0, q=sn, active=active)
    return _sel(use_diff, diff, spec), np.full(ev.n, 3)


# ---------------------------------------------------------------------------------------------------------------------
# refract, getNewRay
# ---------------------------------------------------------------------------------------------------------------------

def _refract(ev, mtl, d, n, draw, active):
    """pt_utils.cl:436-465 -> (direction, draws taken)."""
    ni = mtl[1]
    front = _dot(ev, n, -d)
    into = ev.decide("R.into", front > 0.0, q=front, active=active)
    nl = _sel(into, n, -n)
    m1 = np.where(into, NI_AIR, ni)
    m2 = np.where(into, ni, NI_AIR)
    m = ev.r(m1 / m2)
    cosI = -_dot(ev, nl, d)
    sinT2 = ev.r(ev.r(m * m) * ev.r(1.0 - ev.r(cosI * cosI)))
    tir = ev.decide("R.tir", sinT2 >= 1.0, q=sinT2 - 1.0, active=active)
    with np.errstate(invalid="ignore"):
        sqrtCosT = ev.r(_sqrt(ev.r(1.0 - sinT2)))
    r0 = ev.r(ev.r(m1 - m2) / ev.r(m1 + m2))
    dense = np.where(into, ev.decide("R.dense_in", NI_AIR > ni), ev.decide("R.dense_out", ni > NI_AIR))  # m1 > m2: inputs
    c = np.where(dense, sqrtCosT, cosI)
    reflectance = _fresnel(ev, c, ev.r(r0 * r0))
    rnd = draw(0)
    trans = ev.decide("R.trans", reflectance < rnd, q=reflectance - rnd, active=active & ~tir)
    through = ev.r(m[:, None] * d + ev.r(ev.r(m * cosI) - sqrtCosT)[:, None] * nl)
    mirrored = _reflect(ev, d, nl)
    return _sel(tir, mirrored, _sel(trans, through, mirrored)), np.where(tir, 0, 1)


def new_ray(brdf):
    """getNewRay, pt_brdf.cl:344-378, for one BRDF model: fn( ev, mtl, x ) with x = {origin, dir, normal, t (n,),
    draws (n, DRAWS)} -> {val: (n, 6) {origin, dir}, used: draws taken, add: addDepth}."""
    sampler = _new_ray_schlick if brdf == 0 else _new_ray_shirley_ashikhmin

    def fn(ev, mtl, x):
        origin, d, n, t, draws = x["origin"], x["dir"], x["normal"], x["t"], x["draws"]
        o = ev.r(t[:, None] * d + origin)
        translucent = ev.decide("N.translucent", mtl[0] < 1.0)
        k0 = translucent.astype(np.int64)                 # `d < 1 && d <= rand( seed )`: no draw when d >= 1

        def at(k0):
            return lambda j: draws[np.arange(ev.n), np.minimum(k0 + j, DRAWS - 1)]

        refr = ev.decide("N.refr", translucent & (mtl[0] <= draws[:, 0]))
        dir_r, used_r = _refract(ev, mtl, d, n, at(k0), refr)
        dir_s, used_s = sampler(ev, mtl, d, n, at(k0), ~refr)
        return {"val": np.concatenate([o, _sel(refr, dir_r, dir_s)], axis=1),
                "used": k0 + np.where(refr, used_r, used_s), "add": refr}

    fn.dir_cols = (3, 4, 5)
    return fn


# ---------------------------------------------------------------------------------------------------------------------
# updateColor and the surface step
# ---------------------------------------------------------------------------------------------------------------------

PDF_CUT = float(np.float32(0.00001))          # pathtracing.cl:107 / :141, a float literal


class _Sub:
    """One evaluation seen by a sub-stage that runs more than once in it: the decisions carry a prefix."""

    def __init__(self, ev, prefix, opposite_undefined=False):
        self.ev, self.prefix, self.n, self.rng = ev, prefix, ev.n, ev.rng
        self.opposite_undefined = opposite_undefined

    def r(self, x):
        return self.ev.r(x)

    def decide(self, key, *args, **kwargs):
        return self.ev.decide(self.prefix + key, *args, **kwargs)


def _colours(brdf, mtl):
    """(rgbDiff, rgbSpec) of the material's wire format."""
    at = 4 if brdf == 0 else 8
    return np.asarray(mtl[at:at + 3], np.float64)[None, :], np.asarray(mtl[at + 4:at + 7], np.float64)[None, :]


def _clamp01(x):
    """clamp( x, 0, 1 ) = fmin( fmax( x, 0 ), 1 )."""
    return np.fmin(np.fmax(x, 0.0), 1.0)


def _brdf_colour(ev, brdf, mtl, prefix, out_dir, in_dir, normal, active, cut):
    """What updateColor makes of one BRDF evaluation (pathtracing.cl:105-112 / :120-124 Schlick, :136-150 / :160-173
    Shirley-Ashikhmin): (the colour factor (n, 3), passes — |pdf| > 1e-5, decided only when `cut`).  Schlick: the factor
    fresnel4( u, rgbSpec ) * brdf * d + ( 1 - d ) with brdf = brdf * lambert / pdf; S-A: clamp( brdfColor / maxRGB )."""
    d = mtl[0]
    kd, ks = _colours(brdf, mtl)
    # (a Shirley-Ashikhmin lobe of a large exponent underflows off its peak: spec and pdf are both 0 in binary32 then, and
    # their quotient NaN — _Ev.r models that range)
    res = brdf_eval(brdf)(_Sub(ev, prefix, opposite_undefined=not cut), mtl, {"out": out_dir, "in": in_dir, "normal": normal})["val"]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pdf = res[:, 2] if brdf == 0 else res[:, 3]
        passes = np.ones(ev.n, bool)
        if cut:
            passes = ev.decide(prefix + "pdfcut", np.abs(pdf) > PDF_CUT, q=np.abs(pdf) - PDF_CUT, scale=np.abs(pdf) + PDF_CUT, active=active)
        one_d = ev.r(1.0 - d)
        if brdf == 0:
            lam = np.maximum(_dot(ev, normal, in_dir), 0.0)                 # lambert: max( dot( n, l ), 0 )
            b = ev.r(ev.r(res[:, 0] * lam) / pdf)                           # native_divide
            f4 = _fresnel(ev, res[:, 1][:, None], ks)
            return ev.r(ev.r(ev.r(f4 * b[:, None]) * d) + one_d), passes
        rs = mtl[4]
        spec, diff = ev.r(res[:, 0] / pdf), ev.r(res[:, 1] / pdf)
        fr = _fresnel(ev, res[:, 2], rs)
        brdf_s = ev.r(ev.r(spec[:, None] * ks) * fr[:, None])
        brdf_d = ev.r(ev.r(diff[:, None] * kd) * ev.r(1.0 - rs))
        bc = ev.r(ev.r(ev.r(brdf_s + brdf_d) * d) + one_d)
        max_rgb = np.maximum(1.0, bc.max(axis=1))
        return _clamp01(ev.r(bc / max_rgb[:, None])), passes


def surface_step(brdf):
    """One bounce between the hit and the next ray, pathtracing.cl:281-303: getNewRay with the UNflipped normal, the flip
    of the normal towards the arriving ray (:298-300), updateColor (:89-178) with the flipped one.
    fn( ev, mtl, x ) with x = {dir, normal, color, lightDir, lightRgb (n, 3), lit (n,), draws (n, DRAWS)} ->
    {val: (n, 10) {newDir[3], color after[3], finalColor after starting from 0 [3], secondaryPaths increment},
     used, add}.  The draws start behind `seed += t` (:281), which the caller forms in binary32."""
    sample = new_ray(brdf)

    def fn(ev, mtl, x):
        d, n, color, light_dir, light_rgb = x["dir"], x["normal"], x["color"], x["lightDir"], x["lightRgb"]
        kd, _ = _colours(brdf, mtl)
        zero = np.zeros((ev.n, 3))
        nr = sample(ev, mtl, {"origin": zero, "dir": d, "normal": n, "t": np.zeros(ev.n), "draws": x["draws"]})
        new_dir = nr["val"][:, 3:6]
        front = _dot(ev, n, -d)
        flip = ev.decide("U.flip", front <= 0.0, q=front, active=np.ones(ev.n, bool))
        nf = _sel(flip, -n, n)
        # `if( lightRaySource.x >= 0 )`: on inputs
        lit = ev.decide("U.lit", (x["lit"] != 0.0) & (light_rgb[:, 0] >= 0.0))
        with np.errstate(invalid="ignore", over="ignore"):
            k, passes = _brdf_colour(ev, brdf, mtl, "L.", d, light_dir, nf, lit, True)
            got_light = lit & passes
            if brdf == 0:
                add = ev.r(ev.r(ev.r(color * light_rgb) * kd) * k)          # color * lightRaySource * rgbDiff * ( ... )
            else:
                add = ev.r(ev.r(ev.r(k * light_rgb) * mtl[0]) + ev.r(1.0 - mtl[0]))
            final = _sel(got_light, add, zero)
            k, _ = _brdf_colour(ev, brdf, mtl, "N.", d, new_dir, nf, np.ones(ev.n, bool), False)
            after = ev.r(color * (ev.r(kd * k) if brdf == 0 else k))
        val = np.concatenate([new_dir, after, final, got_light.astype(np.float64)[:, None]], axis=1)
        return {"val": val, "used": nr["used"], "add": nr["add"]}

    fn.dir_cols = (0, 1, 2)
    fn.seed_col, fn.add_col = 10, 11
    # dot( normal, -dir ) is formed by the sampler and again by the flip, from the same operands in the same order
    fn.linked = (("U.flip", "SA.front"), ("U.flip", "R.into"))
    return fn


def brdf_eval(brdf):
    """The BRDF evaluation of one model: fn( ev, mtl, x ) with x = {out, in, normal}; no direction outputs."""
    return brdf_schlick if brdf == 0 else brdf_shirley_ashikhmin


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity, ambiguity, comparison
# ---------------------------------------------------------------------------------------------------------------------

def _ulp_step(v, up):
    return np.nextafter(np.asarray(v, np.float32), np.float32(np.inf if up else -np.inf)).astype(np.float64)


def _perturbations(mtl, x, mtl_keys):
    for k, a in x.items():
        cols = range(a.shape[1]) if a.ndim == 2 else [None]
        for c in cols:
            for up in (False, True):
                b = a.copy()
                if c is None:
                    b[:] = _ulp_step(a, up)
                else:
                    b[:, c] = _ulp_step(a[:, c], up)
                if k == "draws":                          # a draw stays a draw: in [0, 1)
                    b = np.clip(b, 0.0, 1.0 - U)
                yield mtl, dict(x, **{k: b})
    for k in mtl_keys:
        for up in (False, True):
            m = list(mtl)
            m[k] = float(_ulp_step(mtl[k], up))
            yield tuple(m), x


def _spread(a, b):
    """|a - b| per element; 0 where both are the same non-finite value class, inf where only one is finite."""
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    fa, fb = np.isfinite(a), np.isfinite(b)
    d = np.where(fa & fb, d, np.where(fa | fb, np.inf, 0.0))
    return np.where(np.isnan(d), np.inf, d)


class Analysis:
    """The float64 result of one stage for a batch and everything needed to judge a result against it."""

    def __init__(self, fn, mtl, x, mtl_keys, force=None, trials=4, seed=0, flush=False):
        n = next(iter(x.values())).shape[0]
        self.fn, self.mtl, self.x, self.mtl_keys, self.n = fn, tuple(float(v) for v in mtl), x, mtl_keys, n
        self.flush = flush
        ev = _Ev(n, force)
        self.res = fn(ev, self.mtl, x)
        self.dec, self.q = ev.dec, ev.q
        ref = self.res["val"]
        self.delta = np.zeros_like(ref)
        self.dq = {k: np.zeros(n) for k in self.q}
        rng = np.random.default_rng(seed)
        runs = [(m, xx, None) for m, xx in _perturbations(self.mtl, x, mtl_keys)] + [(self.mtl, x, rng)] * trials
        for m, xx, noise in runs:
            ev = _Ev(n, self.dec, noise, flush)
            out = fn(ev, m, xx)
            self.delta = np.maximum(self.delta, _spread(out["val"], ref))
            for k in self.q:
                if k in ev.q:
                    self.dq[k] = np.maximum(self.dq[k], _spread(ev.q[k][0], self.q[k][0]))

    def ambiguous(self, K):
        """{decision: samples whose quantity lies within K error bounds of its threshold, or is undefined (NaN)}."""
        out = {}
        for k, (q, scale) in self.q.items():
            a = np.isnan(q) | (np.isfinite(q) & (np.abs(q) <= K * (U * scale + self.dq[k])))
            if a.any():
                out[k] = a
        return out

    def subset(self, idx, flip):
        """The analysis of samples idx with decision `flip` (or each of a tuple of decisions: branches on one and the same
        computed quantity) taken the other way (the decisions after it recomputed)."""
        keys = (flip,) if isinstance(flip, str) else flip
        force = {k: (~self.dec[k][0][idx], np.zeros(idx.size, bool)) for k in keys}
        return Analysis(self.fn, self.mtl, {k: v[idx] for k, v in self.x.items()}, self.mtl_keys, force, flush=self.flush)

    def scale(self):
        s = np.abs(self.res["val"])
        for c in getattr(self.fn, "dir_cols", ()):
            s[:, c] = 1.0
        return s

    def judge(self, got, K, seeds=None):
        """Per sample: every output within K * ( 2^-24 * scale + Delta ) (non-finite where the reference robustly is),
        the seed after the predicted number of draws, and addDepth."""
        ref, tol = self.res["val"], K * (U * self.scale() + self.delta + TINY)
        val = got[:, :ref.shape[1]].astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok = np.where(np.isfinite(ref), np.abs(val - ref) <= tol, ~np.isfinite(val))
        ok = (ok | np.isinf(self.delta)).all(axis=1)
        if "used" in self.res:
            ok &= got[:, getattr(self.fn, "seed_col", 6)] == seeds[np.arange(self.n), self.res["used"]]
            ok &= got[:, getattr(self.fn, "add_col", 7)] == self.res["add"].astype(np.float32)
        return ok


def check(fn, mtl, x, got, K, mtl_keys, seeds=None, flush=False):
    """Judge `got` (the stage's float32 outputs for inputs x) against the float64 reference.  Returns a dict: ok (per
    sample), ambiguous (per sample: some decision within its error bound), ratio (see _ratio, over the samples
    decided unambiguously), analysis.  flush: the arithmetic under test flushes subnormal results to 0 (the native
    transcendental instructions do), which the rounding trials then model."""
    an = Analysis(fn, mtl, x, mtl_keys, flush=flush)
    ok = an.judge(got, K, seeds)
    amb = np.zeros(an.n, bool)
    for key, a in an.ambiguous(K).items():
        amb |= a
        idx = np.flatnonzero(a & ~ok)
        if idx.size:
            alt = an.subset(idx, key)
            ok[idx] |= alt.judge(got[idx], K, None if seeds is None else seeds[idx])
    # branches on one and the same computed quantity (fn.linked: tuples of decisions) go the other way together
    undecided = an.ambiguous(K)
    for group in getattr(fn, "linked", ()):
        if all(k in undecided for k in group):
            idx = np.flatnonzero(np.logical_and.reduce([undecided[k] for k in group]) & ~ok)
            if idx.size:
                alt = an.subset(idx, group)
                ok[idx] |= alt.judge(got[idx], K, None if seeds is None else seeds[idx])
    return {"ok": ok, "ambiguous": amb, "ratio": _ratio(an, got, amb), "analysis": an}


def _ratio(an, got, amb):
    """|got - ref| / ( 2^-24 * scale + Delta ) over the unambiguous samples, where finite."""
    ref = an.res["val"][~amb]
    val = got[~amb, :ref.shape[1]].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(val - ref) / (U * an.scale()[~amb] + an.delta[~amb] + TINY)
    return r[np.isfinite(r)]


def describe(res, x, got, what, limit=3):
    an, bad = res["analysis"], np.flatnonzero(~res["ok"])
    lines = ["%s: %d of %d samples outside K bounds" % (what, bad.size, an.n)]
    for i in bad[:limit]:
        lines.append("  #%d inputs %s" % (i, {k: np.asarray(v[i]).tolist() for k, v in x.items()}))
        lines.append("     got %s" % (got[i].tolist(),))
        lines.append("     ref %s  delta %s" % (an.res["val"][i].tolist(), an.delta[i].tolist()))
        if "used" in an.res:
            lines.append("     draws used %d, addDepth %d" % (an.res["used"][i], an.res["add"][i]))
    return "\n".join(lines)
