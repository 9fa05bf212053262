"""Float64 references for Phong tessellation (numpy only: no oracle, no device), and the committed case sets.

What is restated here is the DEFINITION of the patch and of a polynomial's roots, not the reference's way of intersecting
it (pt_phongtess.cl:56-212: two planes through the ray, a pencil of conics, a cubic and two quadratics):

  patch_point     S( u, v ) = ( 1 - alpha ) p + alpha sum_i b_i proj_i( p ),  p = u P1 + v P2 + w P3,  b = ( u, v, w ),
                  w = 1 - u - v, proj_i the projection onto the plane through P_i with normal N_i (pt_phongtess.cl:14-26)
  patch_hits      ALL solutions ( u, v, t ) of S( u, v ) = o + t d by Newton's iteration on the 3 x 3 system with the
                  analytic Jacobian ( S is quadratic in ( u, v ) ), started from a barycentric grid; it shares no algebra
                  with the conic method
  decide          the reference's acceptance of a solution (inside the triangle, |tNear| <= t <= min( rayT, tFar ),
                  smallest t; pt_phongtess.cl:183-207) applied to those solutions, and how close any solution lies to a
                  decision boundary — the figures that define the AMBIGUOUS cases
  patch_normal    ns from S_u x S_v, np from the interpolated normals, and the reference's choice between them
                  (pt_utils.cl:246-294)
  cubic_real_roots  the real roots of the polynomial whose coefficients are the float32 inputs: np.roots in float64,
                  polished by Newton in np.longdouble; the conditioning of each root; how far the count is from changing

The start grid: 21 points ( i, j, k ) / 5 of the closed triangle.  Checked once on every committed batch of this module
(random at three alphas, nearly flat, strongly curved, axis, through-the-origin, tNear < 0, interval: 9 batches of 4096)
against the 231-point grid ( i, j, k ) / 20: the decision (hit or miss, t, the ambiguity flag) of no case changes;
test_phong_ref_cpu.py repeats that check on part of one batch in the suite.

Solutions far outside the triangle that no start converges to are of no consequence: a decision only looks at solutions
inside the triangle and, for the ambiguity, next to it.

Item layouts are those of pbr_diag_phong_face / orc_phong_face (n x 32) and pbr_diag_solve_cubic / orc_solve_cubic (n x 4).
"""
import numpy as np

BATCH = 4096
MAX_SOL = 8

# closeness thresholds of the ambiguous set (fixed from what the tolerance of the comparison is, 1e-3 relative in t:
# a solution this close to a boundary may fall on either side of it within that tolerance)
EDGE_TOL = 1e-3        # |min( u, v, w )| of a solution
T_TOL = 2e-3           # |t - boundary| / max( 1, t ) for boundary = |tNear| and min( rayT, tFar ): twice the tolerance in t
SEP_TOL = 2e-3         # two solutions inside the triangle with |t_a - t_b| / max( 1, t ) below this
GRAZE_TOL = 2e-2       # |d . ( S_u x S_v )| / ( |d| |S_u x S_v| ): at 1 / 50 an error in ( u, v ) is magnified 50 times in t
NS_TOL = 2e-2          # |dot( ns, r )|: the choice between the two normals


# ---------------------------------------------------------------------------------------------------------------------
# the patch
# ---------------------------------------------------------------------------------------------------------------------

def _patch(P, N, alpha, u, v, derivs=False):
    """S (and S_u, S_v) for P, N of shape (..., 3, 3) [vertex, xyz], alpha and u, v of shape (...)."""
    w = 1.0 - u - v
    b = np.stack([u, v, w], axis=-1)
    p = np.einsum("...i,...ij->...j", b, P)
    h = ((p[..., None, :] - P) * N).sum(-1)                       # ( p - P_i ) . N_i
    a = alpha[..., None]
    S = p - a * np.einsum("...i,...i,...ij->...j", b, h, N)       # sum b_i = 1: p - alpha sum b_i N_i ( ( p - P_i ) . N_i )
    if not derivs:
        return S
    out = [S]
    for k in (0, 1):
        pk = P[..., k, :] - P[..., 2, :]                          # dp / du, dp / dv
        hk = (pk[..., None, :] * N).sum(-1)
        db = np.zeros(3)
        db[k], db[2] = 1.0, -1.0
        out.append(pk - a * (np.einsum("i,...i,...ij->...j", db, h, N) + np.einsum("...i,...i,...ij->...j", b, hk, N)))
    return out


def patch_point(P, N, u, v, alpha):
    """The definition: ( 1 - alpha ) p + alpha sum_i b_i proj_i( p ).  P, N: (..., 3, 3); u, v, alpha broadcast."""
    P, N = np.asarray(P, np.float64), np.asarray(N, np.float64)
    u, v, alpha = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(v, np.float64), np.asarray(alpha, np.float64))
    w = 1.0 - u - v
    p = u[..., None] * P[..., 0, :] + v[..., None] * P[..., 1, :] + w[..., None] * P[..., 2, :]
    acc = np.zeros_like(p)
    for i, bi in enumerate((u, v, w)):
        n = N[..., i, :]
        proj = p - n * ((p - P[..., i, :]) * n).sum(-1, keepdims=True)
        acc = acc + bi[..., None] * proj
    return (1.0 - alpha)[..., None] * p + alpha[..., None] * acc


def start_grid(div=5):
    pts = [(i / div, j / div) for i in range(div + 1) for j in range(div + 1 - i)]
    return np.array(pts, np.float64)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def patch_hits(P, N, o, d, alpha, div=5, iters=32):
    """All solutions of S( u, v ) = o + t d that Newton's iteration reaches from the start grid.

    P, N: (m, 3, 3); o, d: (m, 3); alpha: (m,).  Returns sol (m, MAX_SOL, 3) of ( u, v, t ), NaN-padded, sorted by t, and
    graze (m, MAX_SOL): |d . ( S_u x S_v )| / ( |d| |S_u x S_v| ) at each solution.
    """
    P, N, o, d = (np.asarray(x, np.float64) for x in (P, N, o, d))
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), P.shape[:1])
    m = P.shape[0]
    g = start_grid(div)
    G = g.shape[0]
    # S is a quadratic polynomial in ( u, v ): S = c0 + c1 u + c2 v + c3 u^2 + c4 u v + c5 v^2, its six coefficients from
    # the definition at six points (exact up to rounding); the iteration runs on that form, the residual that accepts a
    # solution is taken with the definition itself (patch_point)
    at = lambda uu, vv: patch_point(P, N, uu, vv, alpha)
    s00, s10, s01, sh0, s0h, shh = at(0.0, 0.0), at(1.0, 0.0), at(0.0, 1.0), at(0.5, 0.0), at(0.0, 0.5), at(0.5, 0.5)
    c0 = s00
    c3 = 2.0 * (s10 + s00 - 2.0 * sh0)
    c5 = 2.0 * (s01 + s00 - 2.0 * s0h)
    c1 = s10 - s00 - c3
    c2 = s01 - s00 - c5
    c4 = 4.0 * shh - 4.0 * c0 - 2.0 * (c1 + c2) - c3 - c5
    c0, c1, c2, c3, c4, c5 = (c[:, None, :] for c in (c0, c1, c2, c3, c4, c5))
    og, dg = o[:, None, :], d[:, None, :] * np.ones((1, G, 1))
    u = np.broadcast_to(g[:, 0], (m, G)).copy()
    v = np.broadcast_to(g[:, 1], (m, G)).copy()
    dd = (d * d).sum(-1)[:, None]
    scale = np.abs(P).max(axis=(1, 2))[:, None] + np.abs(o).max(-1)[:, None]

    def quad(u, v):
        u3, v3 = u[..., None], v[..., None]
        return (c0 + c1 * u3 + c2 * v3 + c3 * u3 * u3 + c4 * u3 * v3 + c5 * v3 * v3,
                c1 + 2.0 * c3 * u3 + c4 * v3, c2 + c4 * u3 + 2.0 * c5 * v3)

    t = ((quad(u, v)[0] - og) * dg).sum(-1) / dd
    step = np.full((m, G), np.inf)
    c = -dg                                                        # J = [ Su Sv c ], J x = -F by Cramer's rule
    with np.errstate(all="ignore"):
        for _ in range(iters):
            S, Su, Sv = quad(u, v)
            F = S - og - t[..., None] * dg
            bc = _cross(Sv, c)
            det = (Su * bc).sum(-1)
            du = -(F * bc).sum(-1) / det
            dv = -(Su * _cross(F, c)).sum(-1) / det
            dt = -(Su * _cross(Sv, F)).sum(-1) / det
            big = np.maximum(np.abs(du), np.abs(dv))
            damp = np.where(big > 2.0, 2.0 / big, 1.0)             # no wild first steps; Newton proper near a solution
            u, v, t = u + du * damp, v + dv * damp, t + dt * damp
            step = big
        _, Su, Sv = quad(u, v)
        S = patch_point(P[:, None], N[:, None], u, v, alpha[:, None])
        res = np.abs(S - og - t[..., None] * dg).max(-1)
        nrm = _cross(Su, Sv)
        graze = np.abs((nrm * dg).sum(-1)) / np.sqrt((nrm * nrm).sum(-1) * dd)
    # accepted: tiny residual.  A transversal solution also has a tiny last step; at a tangential one (double root) the
    # iteration converges linearly and the residual is of second order in the distance — such a case is grazing anyway.
    ok = np.isfinite(u) & np.isfinite(v) & np.isfinite(t) & (res <= 1e-11 * scale) & (step <= 1e-4)
    sol = np.full((m, MAX_SOL, 3), np.nan)
    gr = np.full((m, MAX_SOL), np.nan)
    for k in range(m):
        idx = np.flatnonzero(ok[k])
        if idx.size == 0:
            continue
        cand = np.stack([u[k, idx], v[k, idx], t[k, idx]], axis=1)
        order = np.argsort(cand[:, 2], kind="stable")
        kept, keptg = [], []
        for j in order:
            c_ = cand[j]
            if all(max(abs(c_[0] - q[0]), abs(c_[1] - q[1])) > 1e-6 for q in kept):
                kept.append(c_)
                keptg.append(graze[k, idx[j]])
        kept, keptg = kept[:MAX_SOL], keptg[:MAX_SOL]
        sol[k, : len(kept)] = kept
        gr[k, : len(kept)] = keptg
    return sol, gr


def decide(sol, graze, t_near, t_far, ray_t):
    """The reference's acceptance applied to the float64 solutions: t (inf: miss), the index of the accepted solution
    (-1), and the ambiguity flag from the closeness figures (module docstring)."""
    u, v, t = sol[..., 0], sol[..., 1], sol[..., 2]
    lo = np.abs(np.asarray(t_near, np.float64))[:, None]
    hi = np.minimum(np.asarray(ray_t, np.float64), np.asarray(t_far, np.float64))[:, None]
    with np.errstate(invalid="ignore"):
        bary = np.minimum(np.minimum(u, v), 1.0 - u - v)
        have = np.isfinite(t)
        inside = have & (bary >= 0.0)
        valid = inside & (t >= lo) & (t <= hi)
        tt = np.where(valid, t, np.inf)
        pick = np.argmin(tt, axis=1)
        t_ref = tt[np.arange(sol.shape[0]), pick]
        pick = np.where(np.isfinite(t_ref), pick, -1)
        rel = np.maximum(1.0, np.abs(t))
        # only solutions that could take part in a decision count: next to the triangle, next to the interval
        near_tri = have & (bary > -EDGE_TOL)
        near_int = (t >= lo - T_TOL * rel) & (t <= hi + T_TOL * rel)
        amb_edge = (have & (np.abs(bary) < EDGE_TOL) & near_int).any(1)
        amb_t = (near_tri & ((np.abs(t - lo) < T_TOL * rel) | (np.abs(t - hi) < T_TOL * rel))).any(1)
        amb_graze = (near_tri & near_int & (graze < GRAZE_TOL)).any(1)
        amb_sep = np.zeros(sol.shape[0], bool)
        for a in range(MAX_SOL):
            for b in range(a + 1, MAX_SOL):
                amb_sep |= near_tri[:, a] & near_tri[:, b] & near_int[:, a] & (np.abs(t[:, a] - t[:, b]) < SEP_TOL * rel[:, a])
    return t_ref, pick, amb_edge | amb_t | amb_graze | amb_sep


def patch_normal(P, N, d, alpha, u, v):
    """(ns, np, the reference's choice, |dot( ns, r )|) at ( u, v ): ns = normalize( S_u x S_v ), np = normalize( u N1 + v N2 +
    w N3 ), r = d - 2 np ( d . np ), the choice dot( ns, r ) < 0 ? ns : np (pt_utils.cl:283-294)."""
    P, N, d = (np.asarray(x, np.float64) for x in (P, N, d))
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), P.shape[:1])
    _, Su, Sv = _patch(P, N, alpha, u, v, derivs=True)
    ns = _cross(Su, Sv)
    ns = ns / np.linalg.norm(ns, axis=-1, keepdims=True)
    w = 1.0 - u - v
    npn = u[:, None] * N[:, 0] + v[:, None] * N[:, 1] + w[:, None] * N[:, 2]
    npn = npn / np.linalg.norm(npn, axis=-1, keepdims=True)
    r = d - 2.0 * npn * (d * npn).sum(-1, keepdims=True)
    s = (ns * r).sum(-1)
    return ns, npn, np.where((s < 0.0)[:, None], ns, npn), np.abs(s)


def split_items(items):
    """(P, N, o, d, rayT, tNear, tFar, alpha) in float64 from n x 32 float32 items."""
    it = np.asarray(items, np.float32).astype(np.float64)
    return (it[:, 0:9].reshape(-1, 3, 3), it[:, 9:18].reshape(-1, 3, 3), it[:, 18:21], it[:, 21:24],
            it[:, 24], it[:, 25], it[:, 26], it[:, 27])


_REF_CACHE = {}


def reference(items, key=None, div=5):
    """dict(t, amb, u, v, normal, ns_dot, sol) for a batch; computed once per `key` and shared (do not modify)."""
    if key is not None and (key, div) in _REF_CACHE:
        return _REF_CACHE[(key, div)]
    P, N, o, d, ray_t, t_near, t_far, alpha = split_items(items)
    sol, graze = patch_hits(P, N, o, d, alpha, div=div)
    t_ref, pick, amb = decide(sol, graze, t_near, t_far, ray_t)
    rows = np.arange(sol.shape[0])
    chosen = sol[rows, np.maximum(pick, 0)]
    hit = pick >= 0
    u = np.where(hit, chosen[:, 0], 1 / 3)
    v = np.where(hit, chosen[:, 1], 1 / 3)
    _, _, normal, ns_dot = patch_normal(P, N, d, alpha, u, v)
    out = dict(t=t_ref, amb=amb, hit=hit, u=u, v=v, normal=normal, ns_dot=ns_dot, sol=sol, graze=graze)
    for a in out.values():
        a.setflags(write=False)
    if key is not None:
        _REF_CACHE[(key, div)] = out
    return out


# ---------------------------------------------------------------------------------------------------------------------
# patch cases
# ---------------------------------------------------------------------------------------------------------------------

def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def _slab(lo, hi, o, d):
    """tNear, tFar of the slab test in float64 (axis-parallel rays: +-inf from the division)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
    t_near = np.fmax.reduce(np.fmin(t1, t2), axis=-1)
    t_far = np.fmin.reduce(np.fmax(t1, t2), axis=-1)
    return t_near, t_far


def _patch_box(P, N, alpha, pad=1e-3):
    """A box around the sampled patch (barycentric grid of 12 subdivisions), padded by `pad` of its diagonal."""
    g = start_grid(12)
    m = P.shape[0]
    S = _patch(P[:, None], N[:, None], alpha[:, None] * np.ones((1, g.shape[0])),
               np.broadcast_to(g[:, 0], (m, g.shape[0])), np.broadcast_to(g[:, 1], (m, g.shape[0])))
    lo, hi = S.min(1), S.max(1)
    ext = np.linalg.norm(hi - lo, axis=-1, keepdims=True) * pad
    return lo - ext, hi + ext


def make_items(rng, n, alpha, spread, directions=None):
    """Random patches and rays as in the feasibility experiment: vertices uniform in [-1, 1]^3, normals = the geometric
    normal + N( 0, spread^2 ) noise, renormalised; rays from 3 - 5 units away towards points of the flat triangle (a
    quarter of them towards points of the triangle scaled by 1.5 about its centroid: clear misses too); the leaf box around
    the sampled patch; rayT = inf.  `spread` is a number or an array of n.  `directions`: n x 3 ray directions to use."""
    P = rng.uniform(-1, 1, (n, 3, 3))
    ng = _unit(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]))
    spread = np.broadcast_to(np.asarray(spread, np.float64), (n,))
    N = _unit(ng[:, None, :] + rng.normal(size=(n, 3, 3)) * spread[:, None, None])
    b = rng.dirichlet([1, 1, 1], n)
    wide = rng.random(n) < 0.25
    b = np.where(wide[:, None], 1 / 3 + 1.5 * (b - 1 / 3), b)
    target = np.einsum("ni,nij->nj", b, P)
    if directions is None:
        directions = -_unit(rng.normal(size=(n, 3)))
    d = np.asarray(directions, np.float64)
    o = target - d * rng.uniform(3, 5, (n, 1))
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), (n,))
    items = np.zeros((n, 32), np.float32)
    items[:, 0:9], items[:, 9:18] = P.reshape(n, 9), N.reshape(n, 9)
    items[:, 18:21], items[:, 21:24] = o, d
    items[:, 21:24] = _unit(items[:, 21:24].astype(np.float64))
    items[:, 24], items[:, 27] = np.inf, alpha
    return set_box(items)


def set_box(items):
    """tNear / tFar from the padded box of the patch the float32 item describes."""
    P, N, o, d, _, _, _, alpha = split_items(items)
    lo, hi = _patch_box(P, N, alpha)
    t_near, t_far = _slab(lo, hi, o, d)
    items[:, 25], items[:, 26] = t_near, t_far
    return items


ALPHAS = (0.3, 0.6, 1.0)


def random_batch(alpha, n=BATCH):
    return make_items(np.random.default_rng(1000 + int(round(alpha * 10))), n, alpha, 0.35)


def nearly_flat_batch(n=BATCH):
    """Normal spread 1e-7 ... 1e-2 around the geometric normal (log-uniform), alpha = 0.6; the first 64: spread 0, three
    EQUAL normals (what checkFaceIntersection would have sent to the flat test).  Returns (items, spread)."""
    rng = np.random.default_rng(2001)
    spread = 10.0 ** rng.uniform(-7, -2, n)
    spread[:64] = 0.0
    return make_items(rng, n, 0.6, spread), spread


def curved_batch(n=BATCH):
    return make_items(np.random.default_rng(2002), n, 0.6, 1.0)


def axis_batch(n=BATCH):
    """Rays along one axis, along the diagonal of two axes and of all three, both signs: getBestRayDomain's ties, and
    1 / 0 in the slab test."""
    rng = np.random.default_rng(2003)
    base = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1], [1, -1, 0], [-1, 1, 1]], np.float64)
    d = _unit(base)[rng.integers(0, len(base), n)] * rng.choice([-1.0, 1.0], (n, 1))
    return make_items(rng, n, 0.6, 0.35, directions=d)


def through_origin_batch(n=BATCH):
    """origin = -4 dir exactly: cross( origin, dir ) = 0 and the first plane's normal n1 is 0 / 0."""
    rng = np.random.default_rng(2004)
    items = make_items(rng, n, 0.6, 0.35)
    d = items[:, 21:24].astype(np.float64)
    shift = -4.0 * d - items[:, 18:21].astype(np.float64)
    for k in range(3):
        items[:, 3 * k: 3 * k + 3] = items[:, 3 * k: 3 * k + 3].astype(np.float64) + shift
    items[:, 18:21] = -4.0 * items[:, 21:24]
    return set_box(items)


def negative_near_batch(n=BATCH):
    """tNear < 0 (the origin inside the leaf's box): the reference accepts only t >= |tNear|."""
    rng = np.random.default_rng(2005)
    items = make_items(rng, n, 0.6, 0.35)
    items[:, 25] = -rng.uniform(0, 6, n)
    return items


def interval_batch(n=BATCH):
    """tFar, rayT and |tNear| just either side of the hit the float64 reference finds: factors 1 +- {1e-6 ... 3e-2} of it
    (those within T_TOL are ambiguous by construction: the hard invariants are what holds them)."""
    rng = np.random.default_rng(2006)
    items = make_items(rng, n, 0.6, 0.35)
    ref = reference(items)
    t = np.where(ref["hit"], ref["t"], 4.0)
    factor = 1.0 + rng.choice([-1.0, 1.0], n) * rng.choice([1e-6, 1e-5, 1e-4, 1e-3, 5e-3, 1e-2, 3e-2], n)
    which = rng.integers(0, 3, n)                # 0: tFar, 1: rayT, 2: tNear (the lower end)
    items[:, 26] = np.where(which == 0, t * factor, items[:, 26])
    items[:, 24] = np.where(which == 1, t * factor, items[:, 24])
    items[:, 25] = np.where(which == 2, t * factor * rng.choice([-1.0, 1.0], n), items[:, 25])
    return items


# ---------------------------------------------------------------------------------------------------------------------
# cubics
# ---------------------------------------------------------------------------------------------------------------------

EPS32 = 2.0 ** -23
COUNT_MARGIN = 16.0    # the count is ambiguous when the discriminant is within this many float32 rounding bounds of 0


def _newton_longdouble(a, r, steps=4):
    a = a.astype(np.longdouble)
    r = r.astype(np.longdouble)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            p = ((a[0] * r + a[1]) * r + a[2]) * r + a[3]
            dp = (3 * a[0] * r + 2 * a[1]) * r + a[2]
            step = np.where(dp != 0, p / dp, 0)
            r = r - np.where(np.isfinite(step), step, 0)
    return r.astype(np.float64)


def cubic_real_roots(a):
    """For ONE polynomial a[0] x^3 + a[1] x^2 + a[2] x + a[3] with float32 coefficients: (roots, cond, expected, margin).

    roots: the real roots, ascending (np.roots in float64, Newton in longdouble); cond[k] = sum |a_i| |r|^(3-i) / |p'( r )|,
    the first-order movement of root k under relative perturbations of the coefficients; expected: the count the branch
    solveCubic takes can return — 3 or 1 (a0 != 0), 2 or 0 (a0 == 0, a1 != 0), 1 (linear), 0; margin: |discriminant| over
    the float32 rounding bound of the discriminant as solveCubic forms it (dis = q^2 + p^3, or p^2 - a3 / a1): below
    COUNT_MARGIN the count is ambiguous.  inf for the linear and the empty case."""
    a = np.asarray(a, np.float32).astype(np.float64)
    a0, a1, a2, a3 = a
    margin = np.inf
    if a0 != 0.0:
        w = a1 / a0 / 3.0
        p0 = a2 / a0 / 3.0 - w * w
        qa, qb = 0.5 * (a2 * w - a3) / a0, w ** 3
        q = qa - qb
        dis = q * q + p0 ** 3
        err_q = EPS32 * (2 * abs(0.5 * a2 * w / a0) + abs(0.5 * a3 / a0) + 3 * abs(qb) + abs(q))
        err_p = EPS32 * (2 * abs(a2 / a0 / 3.0) + 3 * w * w + abs(p0))
        err = 2 * abs(q) * err_q + 3 * p0 * p0 * err_p + EPS32 * (q * q + 2 * abs(p0) ** 3) + 1e-300
        margin = abs(dis) / err
        expected = 3 if dis < 0 else 1
        coeffs = a
    elif a1 != 0.0:
        p = 0.5 * a2 / a1
        dis = p * p - a3 / a1
        err = EPS32 * (3 * p * p + 2 * abs(a3 / a1)) + 1e-300
        margin = abs(dis) / err
        expected = 2 if dis >= 0 else 0
        coeffs = a[1:]
    elif a2 != 0.0:
        expected, coeffs = 1, a[2:]
    else:
        return np.zeros(0), np.zeros(0), 0, np.inf
    with np.errstate(all="ignore"):
        r = np.roots(coeffs)
    # real: imaginary part small against the root (a double root splits into a conjugate pair: such a case is ambiguous)
    real = np.abs(r.imag) <= 1e-6 * np.maximum(np.abs(r), 1e-300)
    r = np.sort(_newton_longdouble(a, r.real[real]))
    with np.errstate(all="ignore"):
        dp = np.abs((3 * a0 * r + 2 * a1) * r + a2)
        cond = (abs(a0) * np.abs(r) ** 3 + abs(a1) * r * r + abs(a2) * np.abs(r) + abs(a3)) / dp
    if len(r) != expected:
        margin = 0.0                                              # numpy's count disagrees with the sign: a multiple root
    return r, cond, expected, margin


def _poly_from_roots(r0, r1, r2, lead):
    return np.stack([lead, -lead * (r0 + r1 + r2), lead * (r0 * r1 + r0 * r2 + r1 * r2), -lead * r0 * r1 * r2], axis=1)


def cubic_batch(n=BATCH):
    """n x 4 float32: cubics with three real roots and with one; a0 = 0 quadratics with two roots and with none;
    a0 = a1 = 0 linear; all zero; roots spread over 1e-3 ... 1e3; random coefficients; the pencil's own kind (tiny leading
    coefficients against the rest)."""
    rng = np.random.default_rng(3001)
    k = n // 8
    sgn = lambda m: rng.choice([-1.0, 1.0], m)
    lead = lambda m: sgn(m) * 10.0 ** rng.uniform(-3, 3, m)
    parts = []
    r = rng.uniform(-10, 10, (k, 3))
    parts.append(_poly_from_roots(r[:, 0], r[:, 1], r[:, 2], lead(k)))                       # three real roots
    r0, re, im = rng.uniform(-10, 10, k), rng.uniform(-10, 10, k), rng.uniform(0.1, 10, k)
    parts.append(np.stack([np.ones(k), -(r0 + 2 * re), 2 * re * r0 + re * re + im * im, -r0 * (re * re + im * im)], axis=1) * lead(k)[:, None])
    r = sgn((k, 3)) * 10.0 ** rng.uniform(-3, 3, (k, 3))                                      # roots spread over 1e-3 ... 1e3
    parts.append(_poly_from_roots(r[:, 0], r[:, 1], r[:, 2], lead(k)))
    parts.append(rng.normal(size=(k, 4)) * 10.0 ** rng.uniform(-3, 3, (k, 1)))                # random coefficients
    q = rng.normal(size=(k, 4))
    q[:, 0] *= 10.0 ** rng.uniform(-8, -2, k)                                                 # a nearly quadratic cubic
    parts.append(q)
    r = sgn((k, 2)) * 10.0 ** rng.uniform(-3, 3, (k, 2))
    l2 = lead(k)
    parts.append(np.stack([np.zeros(k), l2, -l2 * (r[:, 0] + r[:, 1]), l2 * r[:, 0] * r[:, 1]], axis=1))   # quadratic, two roots
    re, im = rng.uniform(-10, 10, k), rng.uniform(0.1, 10, k)
    l2 = lead(k)
    parts.append(np.stack([np.zeros(k), l2, -2 * l2 * re, l2 * (re * re + im * im)], axis=1))  # quadratic, none
    m = n - 7 * k
    lin = np.zeros((m, 4))
    lin[:, 2], lin[:, 3] = lead(m), rng.normal(size=m) * 10.0 ** rng.uniform(-3, 3, m)
    lin[:8] = 0.0                                                                             # all zero
    lin[8:16, 2] = 0.0                                                                        # only the constant
    lin[16:24, 3] = 0.0                                                                       # root 0
    parts.append(lin)
    return np.concatenate(parts).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# cbrt
# ---------------------------------------------------------------------------------------------------------------------

def cbrt_inputs():
    """About 1 M float32: 3900 random mantissas in every binade of both signs, the binade's ends, 2^16 subnormals, perfect
    cubes of the integers up to 2^8 (exact in float32) and of k / 8, +-0, +-inf, NaN."""
    rng = np.random.default_rng(4001)
    expo = np.repeat(np.arange(1, 255, dtype=np.uint32), 3900)
    bits = (expo << 23) | rng.integers(0, 1 << 23, expo.size).astype(np.uint32)
    ends = np.concatenate([(np.arange(1, 255, dtype=np.uint32) << 23), (np.arange(1, 255, dtype=np.uint32) << 23) | 0x7FFFFF])
    sub = rng.integers(1, 1 << 23, 1 << 16).astype(np.uint32)
    sub[:4] = [1, 2, 0x7FFFFF, 0x400000]
    pos = np.concatenate([bits, ends, sub]).view(np.float32)
    k = np.arange(1, 257, dtype=np.float64)
    cubes = np.concatenate([k ** 3, (k / 8) ** 3, (k * 64) ** 3]).astype(np.float32)
    sign = rng.choice(np.float32([-1, 1]), pos.size)
    special = np.float32([0.0, -0.0, np.inf, -np.inf, np.nan])
    return np.concatenate([pos * sign, cubes, -cubes, special])
