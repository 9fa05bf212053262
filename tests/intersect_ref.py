"""A float64 restatement of the primitives of the walk: ray against triangle, box and sphere.

Derived from the reference's OpenCL sources, not from the oracle or the kernels:

  source/opencl/pt_intersect.cl  intersectBox (11-25), intersectSphere (37-77), flatTriAndRayIntersect (92-129)
  source/opencl/pt_bvh.cl        the hit condition of traverse (107-110: intersectBox && tFar > EPSILON5 && ray->t > tNear)
                                 and of traverseShadows (151-154: the same without `ray->t > tNear`)
  source/opencl/pt_header.cl     EPSILON5

Item layouts are those of pbr_diag_intersect / orc_intersect (n x 24 in, n x 4 out).  The machinery is shading_ref's:
every statement is a rounding point (`_Ev.r`), and so are the products and partial sums of a dot or cross product, which
cancel; every branch on a computed quantity is a `decide` with its quantity and the scale of its rounding; tolerances come
from the measured sensitivity (`Analysis`), and where a quantity lies within its bound of the threshold either branch is
accepted (`check`).

The reference's quirks are kept:

  * intersectSphere compares d2 with r, not with r * r (pt_intersect.cl:53), and takes sqrt( r - d2 ) (:57).
  * flatTriAndRayIntersect moves the origin to f = max( 0, tNear - 0.001 ) along the ray (:96-97), tests t against
    EPSILON5 and ray->t BEFORE adding f back (:105-107, :120), and accepts u + v == 1 and u == 0 / v == 0 (:115).
  * A ray in the triangle's plane has determinant 0: invDet is inf, t, u and v are inf or NaN, and since every comparison
    with NaN is false such an item can come out as a "hit" with t = NaN.  Here the float64 result is then non-finite too,
    and a non-finite t of either kind is accepted for it.
  * intersectBox with a direction component of +-0: invDir is +-inf, and ( bb - origin ) * invDir is +-inf for an origin
    off the plane and 0 * inf = NaN for an origin exactly ON it.  fmin / fmax return the other operand when one is NaN
    (OpenCL 6.12.2, C99 7.12.12), so the NaN is DROPPED: with the origin on one plane of the slab the axis contributes the
    other plane's +-inf to both tMin and tMax — which is a miss for that axis (tNear = +inf, or tFar = -inf) — and with the
    origin on both (a flat box) both are NaN, fmin / fmax return NaN, the outer fmax / fmin drop it again and the box is
    decided by the remaining axes alone.  np.fmin / np.fmax have the same semantics and state it below.
"""
import numpy as np

import shading_ref as sr

EPSILON5 = float(np.float32(0.00001))         # pt_header.cl, a float literal
BACKOFF = float(np.float32(0.001))            # pt_intersect.cl:96, a float literal
NO_MTL = ()                                   # these stages read no material


def _mul(ev, a, b):
    return ev.r(a * b)


def dot3(ev, a, b):
    """dot( a, b ) = ( a.x b.x + a.y b.y ) + a.z b.z: three products and two sums, each a rounding point."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = ev.r(a * b)
        return ev.r(ev.r(p[:, 0] + p[:, 1]) + p[:, 2])


def cross3(ev, a, b):
    """cross( a, b ): per component two products and their (cancelling) difference."""
    with np.errstate(invalid="ignore", over="ignore"):
        return ev.r(ev.r(a[:, [1, 2, 0]] * b[:, [2, 0, 1]]) - ev.r(a[:, [2, 0, 1]] * b[:, [1, 2, 0]]))


def abs_dot(a, b):
    """sum |a_i b_i|: what the rounding of dot( a, b ) is relative to."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(a * b).sum(axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# triangle: x = {a, b, c, origin, dir (n, 3), rayT, tNear (n,)} -> val (n, 1) {t, inf = no hit}
# ---------------------------------------------------------------------------------------------------------------------

def triangle(ev, mtl, x, slip=None):
    """pt_intersect.cl:92-129.  slip: a named transcription slip, for the test that the comparison is not vacuous."""
    a, b, c, o, d, rayT, tNear = x["a"], x["b"], x["c"], x["origin"], x["dir"], x["rayT"], x["tNear"]
    on = np.ones(ev.n, bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        back = ev.r(tNear - BACKOFF)
        # fmax( 0, tNear - 0.001 ): a decision on a computed quantity (:96)
        pos = ev.decide("T.backoff", back > 0.0, q=back, scale=np.abs(tNear) + BACKOFF, active=on)
        f = np.where(pos, back, 0.0)
        if slip == "no-backoff":
            f = np.maximum(tNear, 0.0)
        close = ev.r(d * f[:, None] + o)                                     # fma: one rounding (:97)
        e1, e2 = ev.r(b - a), ev.r(c - a)
        tv = ev.r(close - a)
        pv, qv = cross3(ev, d, e2), cross3(ev, tv, e1)
        det = dot3(ev, e1, pv)
        inv = ev.r(1.0 / det)                                                # native_recip (:103)
        t = ev.r(dot3(ev, e2, qv) * inv)
        far = ev.decide("T.rayT", t >= rayT, q=t - rayT, scale=np.abs(t) + np.abs(rayT), active=on)
        near = ev.decide("T.eps", t < EPSILON5, q=t - EPSILON5, scale=np.abs(t) + EPSILON5, active=~far)
        go = ~far & ~near
        u = ev.r(dot3(ev, tv, pv) * inv)
        v = ev.r(dot3(ev, d, qv) * inv)
        s = ev.r(u + v)
        if slip == "u+v>=1":
            over = ev.decide("T.uv", s >= 1.0, q=s - 1.0, scale=1.0 + np.abs(u) + np.abs(v), active=go)
        else:
            over = ev.decide("T.uv", s > 1.0, q=s - 1.0, scale=1.0 + np.abs(u) + np.abs(v), active=go)
        m = np.fmin(u, v)
        neg = ev.decide("T.min", m < 0.0, q=m, scale=np.abs(m), active=go & ~over)
        hit = go & ~over & ~neg
        return {"val": np.where(hit, ev.r(t + f), np.inf)[:, None]}


def triangle_inputs(items):
    r = items.astype(np.float64)
    return {"a": r[:, 0:3], "b": r[:, 3:6], "c": r[:, 6:9], "origin": r[:, 9:12], "dir": r[:, 12:15],
            "rayT": r[:, 15], "tNear": r[:, 16]}


# ---------------------------------------------------------------------------------------------------------------------
# box: x = {min, max, origin, dir (n, 3), rayT (n,)} -> val (n, 4) {closest-hit verdict, any-hit verdict, tNear, tFar}
# ---------------------------------------------------------------------------------------------------------------------

def box(ev, mtl, x):
    """pt_intersect.cl:11-25 with invDir = native_recip( dir ) (pt_bvh.cl:84), tNear = 0 / tFar = INFINITY going in
    (pt_bvh.cl:104-105), and the two hit conditions, pt_bvh.cl:107-110 and :151-154."""
    lo, hi, o, d, rayT = x["min"], x["max"], x["origin"], x["dir"], x["rayT"]
    on = np.ones(ev.n, bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inv = ev.r(1.0 / d)                                                  # 1 / +-0 = +-inf
        t1 = ev.r(ev.r(lo - o) * inv)                                        # 0 * inf = NaN: origin on the plane, dir 0
        t2 = ev.r(ev.r(hi - o) * inv)
        tmin, tmax = np.fmin(t1, t2), np.fmax(t1, t2)                        # a NaN operand is dropped
        tNear = np.fmax(np.fmax(tmin[:, 0], tmin[:, 1]), tmin[:, 2])
        tFar = np.fmin(np.fmin(tmax[:, 0], tmax[:, 1]), np.fmin(tmax[:, 2], np.inf))
        # a difference of two infinities of the same sign is no quantity to decide on: the comparison itself is exact then
        gap = np.where(np.isinf(tNear) | np.isinf(tFar), np.where(tNear <= tFar, np.inf, -np.inf), tFar - tNear)
        fin = lambda v: np.where(np.isfinite(v), np.abs(v), 0.0)
        slab = ev.decide("B.slab", tNear <= tFar, q=gap, scale=fin(tNear) + fin(tFar), active=on)
        eps = ev.decide("B.eps", tFar > EPSILON5, q=np.where(np.isinf(tFar), tFar, tFar - EPSILON5), scale=fin(tFar) + EPSILON5, active=slab)
        cull_q = np.where(np.isinf(tNear) | np.isinf(rayT), np.where(rayT > tNear, np.inf, -np.inf), rayT - tNear)
        cull = ev.decide("B.cull", rayT > tNear, q=cull_q, scale=fin(tNear) + fin(rayT), active=slab & eps)
        anyhit = slab & eps
        return {"val": np.stack([(anyhit & cull).astype(np.float64), anyhit.astype(np.float64), tNear, tFar], axis=1)}


def box_inputs(items):
    r = items.astype(np.float64)
    return {"min": r[:, 0:3], "max": r[:, 3:6], "origin": r[:, 6:9], "dir": r[:, 9:12], "rayT": r[:, 12]}


# ---------------------------------------------------------------------------------------------------------------------
# sphere: x = {pos (n, 3), r (n,), origin, dir (n, 3)} -> val (n, 2) {hit, tNear (0 on a miss)}
# ---------------------------------------------------------------------------------------------------------------------

def sphere(ev, mtl, x, slip=None):
    """pt_intersect.cl:37-77.  The swap of :61-63 never runs: thc is a square root, so t0 <= t1."""
    pos, r, o, d = x["pos"], x["r"], x["origin"], x["dir"]
    on = np.ones(ev.n, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        L = ev.r(pos - o)
        tca = dot3(ev, L, d)
        behind = ev.decide("S.tca", tca < 0.0, q=tca, scale=abs_dot(L, d), active=on)
        ll = dot3(ev, L, L)
        tt = ev.r(tca * tca)
        d2 = ev.r(ll - tt)
        rr = ev.r(r * r) if slip == "d2>r*r" else r
        out = ev.decide("S.d2", d2 > rr, q=d2 - rr, scale=ll + tt + np.abs(rr), active=~behind)
        go = ~behind & ~out
        thc = ev.r(sr._sqrt(ev.r(rr - d2)))
        t0, t1 = ev.r(tca - thc), ev.r(tca + thc)
        inside = ev.decide("S.t0", t0 < 0.0, q=t0, scale=np.abs(tca) + thc, active=go)
        gone = ev.decide("S.t1", t1 < 0.0, q=t1, scale=np.abs(tca) + thc, active=go & inside)
        hit = go & ~(inside & gone)
        return {"val": np.stack([hit.astype(np.float64), np.where(hit, np.where(inside, t1, t0), 0.0)], axis=1)}


def sphere_inputs(items):
    r = items.astype(np.float64)
    return {"pos": r[:, 0:3], "r": r[:, 3], "origin": r[:, 4:7], "dir": r[:, 7:10]}


STAGES = {"triangle": (triangle, triangle_inputs, 1), "box": (box, box_inputs, 4), "sphere": (sphere, sphere_inputs, 2)}


def check(op, items, got, K, flush=False, fn=None):
    """Judge got (n x 4, the hook's output) for the items of stage `op`; see shading_ref.check."""
    stage, inputs, cols = STAGES[op]
    return sr.check(fn or stage, NO_MTL, inputs(items), got[:, :cols], K, (), flush=flush)
