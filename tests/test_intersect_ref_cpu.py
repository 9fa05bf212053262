"""The oracle's primitives of the walk (orc_intersect: triangle, box, sphere) against the float64 restatement of the
reference's formulas (tests/intersect_ref.py): random batches of mixed scale and a fixed set of edge cases per
primitive.  No GPU: this holds the oracle — and with it, bit for bit, the HIP kernels' exact mode — to the reference's
formulas.  The GPU tests (test_gpu_intersect_ref.py) reuse the generators and drivers below.

The random generators keep clear of the decision boundaries (interior points at least 5 % inside, misses at least 5 %
outside, no slivers, no grazing rays): the share of a batch that may be ambiguous is capped at AMBIGUOUS_MAX, a condition
on the inputs.  The boundaries themselves are what the edge sets are for."""
import numpy as np
import pytest

import intersect_ref as ir
import shading_ref as sr
from test_shading_ref_cpu import AMBIGUOUS_MAX, K_EXACT, MEDIAN_MAX, assert_ok, unit

N = 2048
INF = np.float32(np.inf)
EPS = np.float32(0.00001)


def up(v, k=1):
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return v


# ---------------------------------------------------------------------------------------------------------------------
# random batches
# ---------------------------------------------------------------------------------------------------------------------

def _scales(rng, n):
    return 10.0 ** rng.uniform(-3, 3, n)


def random_triangles(rng, n=N):
    """Triangles of mixed scale (1e-3 to 1e3), no slivers; half the rays aimed at an interior point, half at a point of
    the plane outside; from either side (back faces too); tNear of 0 or up to half the distance; rayT infinite, beyond the
    hit, or short of it."""
    s = _scales(rng, n)
    tri = np.empty((n, 3, 3))
    todo = np.arange(n)
    while todo.size:
        t = rng.uniform(-1, 1, (todo.size, 3, 3))
        e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
        e3 = t[:, 2] - t[:, 1]
        area = np.linalg.norm(np.cross(e1, e2), axis=1)
        longest = np.maximum(np.maximum((e1 * e1).sum(1), (e2 * e2).sum(1)), (e3 * e3).sum(1))
        good = area > 0.3 * longest
        tri[todo[good]] = t[good]
        todo = todo[~good]
    tri = (tri + rng.uniform(-2, 2, (n, 1, 3))) * s[:, None, None]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    uv = np.empty((n, 2))
    inside = np.arange(n) < n // 2
    todo = np.arange(n)
    while todo.size:
        cand = np.where(inside[todo, None], rng.uniform(0, 1, (todo.size, 2)), rng.uniform(-1, 2, (todo.size, 2)))
        u, v = cand[:, 0], cand[:, 1]
        margin = np.minimum(np.minimum(u, v), 1 - u - v)
        good = np.where(inside[todo], margin > 0.05, (margin < -0.05) & (np.minimum(np.abs(u), np.abs(v)) > 0.05) & (np.abs(1 - u - v) > 0.05))
        uv[todo[good]] = cand[good]
        todo = todo[~good]
    point = a + uv[:, :1] * (b - a) + uv[:, 1:] * (c - a)
    normal = unit(np.cross(b - a, c - a))
    d = np.empty((n, 3))
    todo = np.arange(n)
    while todo.size:
        cand = unit(rng.normal(size=(todo.size, 3)))
        good = np.abs((cand * normal[todo]).sum(1)) > 0.25
        d[todo[good]] = cand[good]
        todo = todo[~good]
    dist = s * rng.uniform(0.5, 4, n)
    items = np.zeros((n, 24), np.float32)
    items[:, 0:3], items[:, 3:6], items[:, 6:9] = a, b, c
    items[:, 9:12], items[:, 12:15] = point - d * dist[:, None], d
    kind = rng.integers(0, 3, n)
    items[:, 15] = np.select([kind == 0, kind == 1], [np.inf, dist * rng.uniform(1.5, 3, n)], dist * 0.3)
    items[:, 16] = np.where(rng.integers(0, 2, n) == 0, 0.0, dist * rng.uniform(0, 0.5, n))
    return items


def random_boxes(rng, n=N):
    """Boxes of mixed scale; origins inside and outside; rays aimed at an interior point, or anywhere."""
    s = _scales(rng, n)
    centre = s[:, None] * rng.uniform(-2, 2, (n, 3))
    half = s[:, None] * rng.uniform(0.1, 1, (n, 3))
    lo, hi = centre - half, centre + half
    inside = rng.integers(0, 2, n) == 0
    origin = np.where(inside[:, None], lo + rng.uniform(0.1, 0.9, (n, 3)) * (hi - lo),
                      centre + unit(rng.normal(size=(n, 3))) * (s * rng.uniform(2.5, 5, n))[:, None])
    aimed = rng.integers(0, 2, n) == 0
    target = np.where(aimed[:, None], lo + rng.uniform(0.1, 0.9, (n, 3)) * (hi - lo),
                      centre + unit(rng.normal(size=(n, 3))) * (s * rng.uniform(2.5, 6, n))[:, None])
    d = unit(target - origin)
    items = np.zeros((n, 24), np.float32)
    items[:, 0:3], items[:, 3:6], items[:, 6:9], items[:, 9:12] = lo, hi, origin, d
    items[:, 12] = np.where(rng.integers(0, 2, n) == 0, np.inf, s * 10.0 ** rng.uniform(-1, 1, n))
    return items


def random_spheres(rng, n=N):
    """Spheres seen from outside and inside.  The reference compares d2 with r (not r * r), so the surface that counts
    is at sqrt( r ) from the centre; the generator follows that."""
    r = 10.0 ** rng.uniform(-2, 2, n)
    R = np.sqrt(r)
    pos = R[:, None] * rng.uniform(-2, 2, (n, 3))
    inside = rng.integers(0, 2, n) == 0
    origin = pos + unit(rng.normal(size=(n, 3))) * (R * np.where(inside, rng.uniform(0, 0.8, n), rng.uniform(1.5, 4, n)))[:, None]
    aimed = rng.integers(0, 2, n) == 0
    target = pos + unit(rng.normal(size=(n, 3))) * (R * np.where(aimed, rng.uniform(0, 0.8, n), rng.uniform(1.3, 6, n)))[:, None]
    items = np.zeros((n, 24), np.float32)
    items[:, 0:3], items[:, 3], items[:, 4:7], items[:, 7:10] = pos, r, origin, unit(target - origin)
    return items


RANDOM = {"triangle": random_triangles, "box": random_boxes, "sphere": random_spheres}


# ---------------------------------------------------------------------------------------------------------------------
# edge sets
# ---------------------------------------------------------------------------------------------------------------------

DYADIC_POINTS = [(0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (0.25, 0.75), (0.75, 0.25), (0.25, 0.25),
                 (-2.0 ** -10, 0.5), (0.5, -2.0 ** -10), (0.5 + 2.0 ** -10, 0.5), (1 + 2.0 ** -10, 0), (0, 1 + 2.0 ** -10)]


def _tri_item(origin, d, rayT=INF, tNear=0.0, a=(0, 0, 0), b=(1, 0, 0), c=(0, 1, 0)):
    it = np.zeros(24, np.float32)
    it[0:3], it[3:6], it[6:9], it[9:12], it[12:15], it[15], it[16] = a, b, c, origin, d, rayT, tNear
    return it


def triangle_edges():
    """(items, want): want[i] is the exact t of item i (inf: a miss) where binary32 is exact on the dyadic triangle
    (0,0,0)(1,0,0)(0,1,0) — asserted as it is in the exact arithmetic —, NaN where nothing is asserted beyond float64."""
    items, want = [], []

    def add(it, w=np.nan):
        items.append(it)
        want.append(w)

    # on each vertex and edge, inside, and just outside each edge; from above and from below (back face), and from a
    # dyadic distance along a dyadic oblique direction ( u + v == 1 hits, u == 0 and v == 0 hit )
    for x, y in DYADIC_POINTS:
        hit = min(x, y) >= 0 and x + y <= 1
        add(_tri_item((x, y, 1), (0, 0, -1)), 1.0 if hit else np.inf)
        add(_tri_item((x, y, -2), (0, 0, 1)), 2.0 if hit else np.inf)
        add(_tri_item((x, y, 4), (0, 0, -2)), 2.0 if hit else np.inf)
    # the ray in the plane (determinant 0) and a few ulp off it
    for k in (0, 1, -1, 2, -2, 4, -4, 64):
        d = np.array([1, 0, k * 2.0 ** -23])
        add(_tri_item((-1, 0.25, 0), d / np.linalg.norm(d)))
        add(_tri_item((-1, 0.25, 0), (1, 0, k * 2.0 ** -23)))
    add(_tri_item((0.25, 0.25, 0), (1, 0, 0)))
    add(_tri_item((-1, -1, 0), (0.6, 0.8, 0)))
    # t one ulp either side of EPSILON5, and of rayT: t is the dyadic height exactly
    for h in (up(EPS, -1), EPS, up(EPS, 1), up(EPS, -8), up(EPS, 8)):
        add(_tri_item((0.25, 0.25, h), (0, 0, -1)), float(h) if h >= EPS else np.inf)
    for rayT in (up(1, -1), 1.0, up(1, 1), up(1, -8), up(1, 8)):
        add(_tri_item((0.25, 0.25, 1), (0, 0, -1), rayT=rayT), 1.0 if np.float32(1) < rayT else np.inf)
    # tNear: f = max( 0, tNear - 0.001 ), the tests on t are taken before f is added back
    for tNear in (0.0, 0.001, up(0.001, 1), up(0.001, -1), 0.002, 1e3, -1.0, -1e3, 2.0, 2.0005, 2.00099, 2.001, 2.002, 1.9995):
        add(_tri_item((0.25, 0.25, 2), (0, 0, -1), tNear=tNear))
        add(_tri_item((0.3, 0.3, 2), (0, 0, -1), rayT=2.5, tNear=tNear))
    # zero area: three times one point, and three points of a line
    add(_tri_item((0.25, 0.25, 1), (0, 0, -1), a=(0, 0, 0), b=(0, 0, 0), c=(0, 0, 0)))
    add(_tri_item((0.25, 0, 1), (0, 0, -1), a=(0, 0, 0), b=(1, 0, 0), c=(2, 0, 0)))
    add(_tri_item((0.25, 0.1, 1), (0, 0, -1), a=(0, 0, 0), b=(1, 0, 0), c=(2, 0, 0)))
    # the same triangle at other scales, hit obliquely from the back
    for s in (1e-3, 1e3):
        d = unit(np.array([[0.3, -0.2, 1.0]]))[0]
        p = np.array([0.2, 0.3, 0.0]) * s
        add(_tri_item(p - d * 2 * s, d, a=(0, 0, 0), b=(s, 0, 0), c=(0, s, 0)))
    return np.array(items, np.float32), np.array(want, np.float64)


def _box_item(lo, hi, origin, d, rayT=INF):
    it = np.zeros(24, np.float32)
    it[0:3], it[3:6], it[6:9], it[9:12], it[12] = lo, hi, origin, d, rayT
    return it


def box_edges():
    """(items, differ): differ[i] — the closest-hit and the any-hit verdict of item i differ (the `rayT > tNear` cull
    alone separates them: only the items built for it have a finite rayT)."""
    items, differ = [], []

    def add(it, dif=False):
        items.append(it)
        differ.append(dif)

    # a direction component of +0 and -0 in each axis, the origin inside the slab, outside it, and exactly on either plane
    for k in range(3):
        k1, k2 = (k + 1) % 3, (k + 2) % 3
        for zero in (0.0, -0.0):
            for ok in (0.5, 1.5, -0.5, 0.0, 1.0, up(0, 1), up(1, -1), up(1, 1), -up(0, 1)):
                o, d = np.zeros(3), np.zeros(3)
                o[k], o[k1], o[k2] = ok, -0.3, -0.4
                d[k], d[k1], d[k2] = zero, 0.6, 0.8
                add(_box_item((0, 0, 0), (1, 1, 1), o, d))
            # two zero components: an axis-parallel ray, through the box and along a face
            for ok in (0.5, 0.0, 1.0, 1.5):
                o, d = np.full(3, ok), np.zeros(3)
                o[k1] = -1.0
                d[k], d[k1], d[k2] = zero, 1.0, zero
                add(_box_item((0, 0, 0), (1, 1, 1), o, d))
        # a flat box in this axis: crossed, and from within its plane
        lo, hi = np.zeros(3), np.ones(3)
        lo[k] = hi[k] = 0.5
        for o_k, d_k in ((-1.0, 1.0), (2.0, -1.0), (0.5, 0.0), (0.5, -0.0), (0.25, 0.0), (0.5, 1.0)):
            o, d = np.zeros(3), np.zeros(3)
            o[k], o[k1], o[k2] = o_k, 0.5 - 0.3 * 1.5 * abs(d_k) - 0.3 * (d_k == 0), 0.5 - 0.4 * 1.5 * abs(d_k) - 0.4 * (d_k == 0)
            d[k], d[k1], d[k2] = d_k, 0.3, 0.4
            add(_box_item(lo, hi, o, unit(d[None])[0] if d_k else d * 2))
    # the origin inside
    rng = np.random.default_rng(8)
    for d in unit(rng.normal(size=(8, 3))):
        add(_box_item((0, 0, 0), (1, 1, 1), (0.5, 0.25, 0.75), d))
    # tFar either side of EPSILON5: the box [-1, 0] left at x = 0 from x = -h, tFar = h exactly
    for h in (up(EPS, -1), EPS, up(EPS, 1), up(EPS, -8), up(EPS, 8), 0.0):
        add(_box_item((-1, 0, 0), (0, 1, 1), (-h, 0.5, 0.5), (1, 0, 0)))
    # rayT either side of tNear = 1: the two verdicts differ here, and only here
    for rayT in (up(1, -1), 1.0, up(1, 1), up(1, -8), up(1, 8), 0.5, 2.0):
        add(_box_item((0, 0, 0), (1, 1, 1), (-1, 0.5, 0.5), (1, 0, 0), rayT=rayT), dif=not np.float32(rayT) > 1)
    # ... with the origin inside tNear is negative and any rayT >= 0 passes
    add(_box_item((0, 0, 0), (1, 1, 1), (0.5, 0.5, 0.5), (1, 0, 0), rayT=0.0))
    # the box behind the ray
    add(_box_item((0, 0, 0), (1, 1, 1), (2, 0.5, 0.5), (1, 0, 0)))
    add(_box_item((0, 0, 0), (1, 1, 1), (2, 2, 2), unit(np.array([[1.0, 1, 1]]))[0]))
    # other scales
    for s in (1e-3, 1e3):
        add(_box_item((0, 0, 0), (s, s, s), (-s, 0.5 * s, 0.25 * s), unit(np.array([[1.0, 0.1, 0.2]]))[0]))
    return np.array(items, np.float32), np.array(differ, bool)


def _sphere_item(pos, r, origin, d):
    it = np.zeros(24, np.float32)
    it[0:3], it[3], it[4:7], it[7:10] = pos, r, origin, d
    return it


def sphere_edges():
    items = []
    for r in (0.25, 4.0):
        R = float(np.sqrt(r))
        # tca either side of 0, inside the sphere
        for x0 in (0.0, up(0, 1), -up(0, 1), 2.0 ** -24, -2.0 ** -24, 1e-3, -1e-3):
            items.append(_sphere_item((0, 0, 0), r, (x0, 0.3 * R, 0), (1, 0, 0)))
        # d2 either side of r: the ray passes the centre at distance y, d2 = y^2
        for x0 in (-1.0, -5.0):
            for y in (R, up(R, -1), up(R, 1), up(R, -64), up(R, 64), 0.8 * R, 1.5 * R, 0.6 * r, r, up(r, 1), up(r, -1), 0.5 * (r + R)):
                items.append(_sphere_item((0, 0, 0), r, (x0, y, 0), (1, 0, 0)))
        # the origin inside, in several directions; on the surface, looking in, out and along it
        for d in unit(np.random.default_rng(9).normal(size=(6, 3))):
            items.append(_sphere_item((0, 0, 0), r, (0.1 * R, 0.1 * R, 0), d))
        for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0.6, 0.8, 0), (-0.6, 0.8, 0)):
            items.append(_sphere_item((0, 0, 0), r, (-R, 0, 0), d))
        # centre on the origin of the ray
        items.append(_sphere_item((1, 2, 3), r, (1, 2, 3), (0, 0, 1)))
    return np.array(items, np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------

class Prims:
    """The implementation under test: fn( op, items ) -> n x 4; the oracle here, the device in test_gpu_intersect_ref.py."""

    def __init__(self, fn, median_max=MEDIAN_MAX, ambiguous_max=AMBIGUOUS_MAX, flush=False, exact=True):
        self.fn, self.median_max, self.ambiguous_max, self.flush, self.exact = fn, median_max, ambiguous_max, flush, exact

    def case(self, op, items, K, random_batch=False):
        got = self.fn(op, items)
        res = ir.check(op, items, got, K, self.flush)
        res["got"] = got
        cols = ir.STAGES[op][2]
        assert_ok(res, op, ir.STAGES[op][1](items), got[:, :cols], random_batch, self.median_max)
        return res


def summary(what, res):
    med = float(np.median(res["ratio"])) if res["ratio"].size else 0.0
    top = float(res["ratio"].max()) if res["ratio"].size else 0.0
    share = float(res["ambiguous"].mean())
    print("%s: median error / bound %.3g, largest %.3g, ambiguous share %.3g (%d of %d)" % (
        what, med, top, share, int(res["ambiguous"].sum()), res["ambiguous"].size))
    return med, top, share


def run_random(prims, op, K, seed=0):
    items = RANDOM[op](np.random.default_rng(700 + 10 * seed + ir.STAGES[op][2]))
    res = prims.case(op, items, K, random_batch=True)
    _, _, share = summary("%s, random batch" % op, res)
    assert share <= prims.ambiguous_max, "%s: %d samples of %d ambiguous" % (op, int(res["ambiguous"].sum()), items.shape[0])
    return res


def run_edges(prims, op, K):
    if op == "triangle":
        items, want = triangle_edges()
        res = prims.case(op, items, K)
        if prims.exact:                      # binary32 is exact on the dyadic items: the verdict itself, and t
            known = ~np.isnan(want)
            got = res["got"][known, 0].astype(np.float64)
            assert np.array_equal(got, want[known]), "dyadic triangle: items %s" % np.flatnonzero(known)[got != want[known]].tolist()
    elif op == "box":
        items, differ = box_edges()
        res = prims.case(op, items, K)
        if prims.exact:
            got = res["got"]
            assert np.array_equal(got[:, 0] != got[:, 1], differ), "closest-hit and any-hit verdicts: items %s" % np.flatnonzero((got[:, 0] != got[:, 1]) != differ).tolist()
            assert (got[differ, 1] == 1).all() and (got[differ, 0] == 0).all()
    else:
        items = sphere_edges()
        res = prims.case(op, items, K)
    summary("%s, edge set of %d" % (op, items.shape[0]), res)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# the oracle as the implementation under test
# ---------------------------------------------------------------------------------------------------------------------

def oracle_prims(oracle):
    return Prims(oracle.intersect)


OPS = ["triangle", "box", "sphere"]


@pytest.mark.parametrize("op", OPS)
def test_oracle_random_batches_match_float64(oracle, op):
    run_random(oracle_prims(oracle), op, K_EXACT)


@pytest.mark.parametrize("op", OPS)
def test_oracle_edge_set_matches_float64(oracle, op):
    run_edges(oracle_prims(oracle), op, K_EXACT)


@pytest.mark.parametrize("op", OPS)
def test_reference_sees_a_transcription_slip(op):
    """Not vacuous: the float64 result rounded to binary32 passes; one relative 1e-5 off fails on most samples."""
    items = RANDOM[op](np.random.default_rng(3))
    fn, inputs, cols = ir.STAGES[op]
    an = sr.Analysis(fn, ir.NO_MTL, inputs(items), ())
    exact = an.res["val"].astype(np.float32)
    assert an.judge(exact, K_EXACT).mean() > 0.999
    finite = np.isfinite(exact).all(axis=1) & (exact[:, -1] != 0)      # a miss has nothing to be off by
    assert finite.mean() > 0.3
    slipped = exact * np.float32(1 + 1e-5)
    if op != "triangle":
        slipped[:, 0] = exact[:, 0]                                    # the verdicts are not what slips
    if op == "box":
        slipped[:, 1] = exact[:, 1]
    assert an.judge(slipped, K_EXACT)[finite].mean() < 0.5


def _slip_output(fn, op, items, slip):
    ev = sr._Ev(items.shape[0])
    val = fn(ev, ir.NO_MTL, ir.STAGES[op][1](items), slip=slip)["val"].astype(np.float32)
    out = np.zeros((items.shape[0], 4), np.float32)
    out[:, :val.shape[1]] = val
    return out


def test_named_slips_fail_on_the_edge_sets():
    """Three slips a transcription could make, each caught by the edge set of its primitive: the sphere's d2 against
    r * r, the triangle without the 0.001 back-off, and u + v >= 1 as the miss condition (which float64 alone cannot see
    — on the edge either branch is within its bound — and the dyadic verdicts do)."""
    items = sphere_edges()
    assert ir.check("sphere", items, _slip_output(ir.sphere, "sphere", items, None), K_EXACT)["ok"].all()
    assert not ir.check("sphere", items, _slip_output(ir.sphere, "sphere", items, "d2>r*r"), K_EXACT)["ok"].all()
    items, want = triangle_edges()
    known = ~np.isnan(want)
    good = _slip_output(ir.triangle, "triangle", items, None)
    assert ir.check("triangle", items, good, K_EXACT)["ok"].all()
    assert np.array_equal(good[known, 0].astype(np.float64), want[known])
    assert not ir.check("triangle", items, _slip_output(ir.triangle, "triangle", items, "no-backoff"), K_EXACT)["ok"].all()
    slipped = _slip_output(ir.triangle, "triangle", items, "u+v>=1")
    assert not np.array_equal(slipped[known, 0].astype(np.float64), want[known])
