"""Rays chosen for the edges of the closest-hit and the any-hit walk, built from the tree they are for (numpy only).

Two hand-made scenes whose every coordinate is a small dyadic number, so that each slab distance and each Moeller-Trumbore t
of the rays below is exact in binary32 and a ray can be put ON an edge of a compare, not near it:

  lanes   some twenty nodes.  Every class has a lane of its own, 8 apart in y: a ray along +x at y = Y meets the boxes and the
          faces of lane Y and misses every other lane's in the y slab.  Node 1 holds the lanes of the first group, a later
          container those of the second, a leaf is the last record — so a ray of the second group misses node 1 and ends on
          the last record, one of the first ends through the miss link -1 of the second container.  With lights there is an
          orb on two lanes (radius word 0.25: intersectSphere compares d2 with r and takes sqrt( r - d2 ) = 0.5).
  chain   hand_scenes' chain300 (603 nodes) under boxes of this module: leaf j holds x in [j, 400], the container behind
          it x in [j + 1, 400].  The ray along +y at x = i + 1/2 walks i pairs, tests every leaf on its way, hits leaf i's
          faces at y = 5 and leaves through the miss link of container i: lane i of a wave departs in visit 2 i + 2.  Leaf
          0's one face spans the whole chain at y = 7: a blocker in the FIRST leaf for tLight = 8, none for tLight = 6, where
          the blocker is in the LAST leaf the ray enters — the face-test count says where the walk stopped.

Every constructor returns a RaySet: rays (n, 6), t0 (n,) — what hit.t starts from: tLight for the any-hit walk —, and a boolean
mask per class.  tests/test_walk_rays_cpu.py asserts each class's defining condition on the inputs with slab32 / tri_t32
below, which restate intersectBox (pt_intersect.cl:11-25) and flatTriAndRayIntersect's t (:92-113) in binary32.

random_set() draws a few thousand ordinary rays with a random tLight for any scene; shadow_truth64() decides them in float64
over all faces with walk_truth's margins.
"""
import numpy as np

import hand_scenes
import refit_scenes
import walk_truth as wt
from test_gpu_shading_ref import NATIVE_SCALE          # 32: what the native arithmetic's roundings are to the exact one's

F = np.float32
INF = F(np.inf)
EPSILON5 = F(0.00001)
EPS_UP, EPS_DOWN = np.nextafter(EPSILON5, F(1)), np.nextafter(EPSILON5, F(0))
PITCH = 8.0                  # lanes are 8 apart in y; a lane's boxes and faces span y in [Y - 1, Y + 3], z in [-1, 3]
ORB_X, ORB_R = 4.0, 0.25     # the orbs' centres lie on their lanes' rays; sqrt( 0.25 ) = 0.5: the ray enters at x = 3.5
ORB_NEAR = F(3.5)


def up(x):
    return np.nextafter(F(x), INF)


def down(x):
    return np.nextafter(F(x), -INF)


class RaySet:
    def __init__(self):
        self._rays, self._t0, self._names = [], [], []

    def add(self, name, origin, direction, t0=np.inf):
        self._rays.append(list(origin) + list(direction))
        self._t0.append(t0)
        self._names.append(name)
        return self

    def done(self):
        self.rays = np.array(self._rays, np.float32).reshape(-1, 6)
        self.t0 = np.array(self._t0, np.float32)
        names = np.array(self._names)
        self.classes = {k: names == k for k in dict.fromkeys(self._names)}
        self.n = self.rays.shape[0]
        return self


# ---- the restatements ---------------------------------------------------------------------------------------------------

def slab32(lo, hi, origin, direction):
    """intersectBox in binary32 with invDir = 1 / dir: (tNear, tFar, NaN axes) of rays (n, 3) against ONE box, or boxes
    (n, 3).  fmin / fmax drop a NaN operand; tFar keeps the reference's fmin( ., INFINITY )."""
    lo, hi, o, d = (np.asarray(v, np.float32) for v in (lo, hi, origin, direction))
    with np.errstate(all="ignore"):
        inv = F(1.0) / d
        t1, t2 = (lo - o) * inv, (hi - o) * inv
        tmin, tmax = np.fmin(t1, t2), np.fmax(t1, t2)
        near = np.fmax(np.fmax(tmin[..., 0], tmin[..., 1]), tmin[..., 2])
        far = np.fmin(np.fmin(tmax[..., 0], tmax[..., 1]), np.fmin(tmax[..., 2], INF))
    return near, far, (np.isnan(t1) | np.isnan(t2)).sum(axis=-1)


def box_hit32(near, far, ray_t, anyhit):
    """pt_bvh.cl:107-110 / :151-154 on slab32's values."""
    with np.errstate(invalid="ignore"):
        hit = (near <= far) & (far > EPSILON5)
        return hit if anyhit else hit & (ray_t > near)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _dot(a, b):
    return _fma(a[..., 2], b[..., 2], _fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def _cross(a, b):
    return np.stack([_fma(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])), _fma(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                     _fma(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], axis=-1)


def tri_t32(tri, origin, direction, t_near):
    """flatTriAndRayIntersect's two distances in binary32 (fused dot and cross as the oracle's table has them): (t' — measured
    from the origin moved to max( 0, tNear - 0.001 ), the value compared with EPSILON5 and ray.t —, t' + f — the value
    returned), and whether u, v pass.  tri (n, 3, 3) or (3, 3)."""
    tri, o, d = (np.asarray(v, np.float32) for v in (tri, origin, direction))
    with np.errstate(all="ignore"):
        f = np.fmax(F(0.0), np.asarray(t_near, np.float32) - F(0.001))
        close = _fma(f[..., None], d, o)
        e1, e2 = tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :]
        tv = close - tri[..., 0, :]
        p, q = _cross(d, e2), _cross(tv, e1)
        inv = F(1.0) / _dot(e1, p)
        t = _dot(e2, q) * inv
        u, v = _dot(tv, p) * inv, _dot(d, q) * inv
        inside = ~((u + v > F(1.0)) | (np.fmin(u, v) < F(0.0)))
    return t, t + f, inside


def sphere_near32(pos, r, origin, direction):
    """intersectSphere's tNear in binary32 for a ray that starts outside and goes through: tca - sqrt( r - d2 )."""
    L = np.asarray(pos, np.float32) - np.asarray(origin, np.float32)
    d = np.asarray(direction, np.float32)
    tca = _dot(L, d)
    d2 = _dot(L, L) - tca * tca
    with np.errstate(invalid="ignore"):
        return tca - np.sqrt(F(r) - d2), d2


# ---- scenes -------------------------------------------------------------------------------------------------------------

def _scene(pbr, bvh, tris, lights):
    """A refit_scenes.Scene of hand-made nodes and triangles (faces x 3 x 3): three vertices and one normal set per face."""
    faces = tris.shape[0]
    vertices, normals = np.zeros((3 * faces, 4), np.float32), np.zeros((3 * faces, 4), np.float32)
    vertices[:, :3] = tris.reshape(-1, 3)
    n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]).astype(np.float64)
    normals[:, :3] = np.repeat(n / np.linalg.norm(n, axis=1, keepdims=True), 3, axis=0)
    facesV = np.zeros((faces, 4), np.uint32)
    facesV[:, :3] = np.arange(3 * faces).reshape(faces, 3)
    arrays = {"bvh": np.ascontiguousarray(bvh, np.float32), "facesV": facesV, "facesN": facesV.copy(), "vertices": vertices, "normals": normals,
              "materials": np.array(hand_scenes.MATERIALS[1], np.float32),
              "lights": np.array(lights, np.float32).reshape(-1, 12)}
    cfg = pbr.Config()
    cfg.width, cfg.height, cfg.brdf, cfg.shadow_rays = hand_scenes.WIDTH, hand_scenes.HEIGHT, 1, 0
    cfg.max_depth, cfg.max_added_depth, cfg.samples = hand_scenes.DEPTH, 0, 1
    cfg.anti_aliasing, cfg.phong_tessellation = 0.0, 0.0
    cfg.sky_light[0], cfg.sky_light[1], cfg.sky_light[2], cfg.sky_light[3] = 0.75, 0.5, 0.25, 0.0
    cfg.tile_world, cfg.tile_rank = 1, 0
    flat = np.zeros(faces, bool)
    sc = refit_scenes.Scene(pbr, arrays, cfg, hand_scenes.camera(pbr, vertices, flat), pbr.pixel_dimension(hand_scenes.WIDTH, hand_scenes.HEIGHT),
                            pbr.frame_seeds(0, hand_scenes.FRAMES))
    sc.flat = flat
    return sc


def _flatten(tree, tris):
    """Nested ("c", box | None, [children]) / ("l", box, [triangle, ...]) -> wire nodes in depth-first order; a container
    without a box gets its children's union.  Triangles are appended to `tris` in leaf order."""
    rows = []

    def walk(node):
        at = len(rows)
        rows.append(None)
        if node[0] == "l":
            first = len(tris)
            tris.extend(node[2])
            assert len(node[2]) in (1, 2)
            lo, hi = node[1]
            rows[at] = [*lo, first, *hi, first + 1 if len(node[2]) == 2 else -1]
            return np.array(lo, np.float64), np.array(hi, np.float64)
        boxes = [walk(child) for child in node[2]]
        lo, hi = node[1] if node[1] is not None else (np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0))
        rows[at] = [*lo, -1, *hi, len(rows)]         # the miss link: where the subtree ends
        return np.array(lo, np.float64), np.array(hi, np.float64)

    walk(tree)
    bvh = np.array(rows, np.float32)
    containers = bvh[:, 3] == -1
    bvh[containers & (bvh[:, 7] >= len(rows)), 7] = -1      # ... and -1 when that is the end of the array
    return bvh


def _face_x(c, Y):
    """A triangle in the plane x = c that the ray ( ., Y, 0 ) along x meets at u = v = 1 / 4; edges ( 0, 4, 0 ) and ( 0, 0, 4 )
    make every product of Moeller-Trumbore a scaling by a power of two: t = c - origin.x exactly."""
    return [[c, Y - 1, -1], [c, Y + 3, -1], [c, Y - 1, 3]]


def _box_x(x0, x1, Y):
    return ([x0, Y - 1, -1], [x1, Y + 3, 3])


# the lanes: name -> Y.  First group under node 1, second group under a later container.
LANES = {"two_face": 0.0, "tie": 8.0, "equal_t": 16.0, "cull": 24.0, "after_hit": 32.0,
         "far_box": 48.0, "orb_front": 56.0, "orb_behind": 64.0, "flat_leaf": 72.0, "flat_container": 80.0, "nan": 88.0, "corner": 96.0}
FIRST_GROUP = ("two_face", "tie", "equal_t", "cull", "after_hit")


def lanes_scene(pbr, lights):
    key = ("walk_rays.lanes", bool(lights))
    if key not in hand_scenes._cache:
        Y = LANES
        leaf = lambda x0, x1, lane, *cs: ("l", _box_x(x0, x1, Y[lane]), [_face_x(c, Y[lane]) for c in cs])
        first = ("c", None, [
            leaf(-1, 3, "two_face", 2, 1),          # the first face blocks, the second — nearer — is still tested and kept
            leaf(-1, 3, "tie", 2),                  # one face at t = 2 ...
            leaf(-1, 4, "tie", 3),                  # ... and a leaf behind it: reached only if the walk goes on
            leaf(-1, 3, "equal_t", 2, 2),           # two faces of one leaf at the same t
            leaf(2, 3, "cull", 2.5),                # tNear = 2 for a ray from x = 0
            leaf(-1, 3, "after_hit", 2),            # a real hit at t = 2 ...
            leaf(2, 3, "after_hit", 2.5),           # ... and a later box with tNear = 2
        ])
        second = ("c", None, [
            leaf(10, 11, "far_box", 10.5),          # tNear = 10: beyond a light at 4
            leaf(-1, 7, "orb_front", 6),            # a face behind the orb at 4 ...
            leaf(-1, 3, "orb_front", 2),            # ... and, later, one in front of it
            leaf(-1, 7, "orb_behind", 6),
            leaf(0, 0, "flat_leaf", 0),             # a leaf's box flat in x = 0
            ("c", _box_x(0, 0, Y["flat_container"]), [leaf(-1, 3, "flat_container", 2), leaf(-1, 3, "flat_container", 2.5)]),
            leaf(0, 1, "nan", 0.5),
            ("l", ([6, Y["nan"], 0], [6, Y["nan"], 0]), [_face_x(6, Y["nan"])]),       # a box that is one point
            ("l", ([2, Y["corner"] + 1, -1], [3, Y["corner"] + 2, 3]), [_face_x(2.5, Y["corner"])]),      # the last record
        ])
        tris = []
        bvh = _flatten(("c", None, [first, second]), tris)
        orbs = [[ORB_X, Y[lane], 0, 0, 4.0, 3.5, 3.0, 0, 2, ORB_R, 0, 0] for lane in ("orb_front", "orb_behind")] if lights else []
        sc = _scene(pbr, bvh, np.array(tris, np.float32), orbs)
        sc.second = int(bvh[1, 7])                  # the second group's container
        hand_scenes._cache[key] = sc
    return hand_scenes._cache[key]


def lanes_rays(anyhit, lights):
    """The edge classes of one walk on the lanes scene."""
    s, Y = RaySet(), LANES
    X = (1.0, 0.0, 0.0)
    light = lambda t: t if anyhit else np.inf          # the closest-hit walk starts from +inf unless a class says otherwise
    # both walks: tFar == EPSILON5 exactly and one place to either side, on a leaf box and on a container box (tNear == tFar)
    for lane in ("flat_leaf", "flat_container"):
        for name, e in (("tfar_eps", EPSILON5), ("tfar_eps_up", EPS_UP), ("tfar_eps_down", EPS_DOWN)):
            for sign in (1.0, -1.0):
                s.add("%s_%s" % (name, lane), (-sign * e, Y[lane], 0.0), (sign, 0.0, 0.0), light(8.0))
    # tNear == tFar at a corner: ( 1, 1, 0 ) meets x in [2, 3] over t in [2, 3] and y in [Y + 1, Y + 2] over t in [1, 2]
    s.add("corner", (0.0, Y["corner"], 0.0), (1.0, 1.0, 0.0), light(8.0))
    # origin in a slab plane of a zero direction component: 0 * inf = NaN terms in one, two and three axes; and a flat box met in its plane
    lo = np.array([0.0, Y["nan"] - 1, -1.0])
    for sz in (0.0, -0.0):
        s.add("nan1", (0.0, Y["nan"], -2.0), (sz, sz, 1.0), light(8.0))
        s.add("nan2", (0.0, Y["nan"] - 1, -2.0), (sz, -sz, 1.0), light(8.0))
        s.add("nan3", lo, (sz, sz, sz), light(8.0))
        s.add("nan3", lo, (sz, -sz, sz), light(8.0))
        # ... and every one of the six terms: the reference's tFar is fmin( NaN, INFINITY ) = inf where a min3 of three NaN is NaN
        s.add("nan_all", (6.0, Y["nan"], 0.0), (sz, sz, sz), light(8.0))
        s.add("flat_in_plane", (0.0, Y["flat_leaf"], -2.0), (sz, sz, 1.0), light(8.0))
        s.add("flat_in_plane", (0.0, Y["flat_leaf"], -2.0), (-sz, sz, 1.0), light(8.0))
    # zero direction components of both signs on a ray that hits
    for zy in (0.0, -0.0):
        for zz in (0.0, -0.0):
            s.add("zero_signs", (0.0, Y["tie"], 0.0), (1.0, zy, zz), light(8.0))
    # node 1 missed (every ray of the second group) / the walk's two ends are asserted on the whole set
    s.add("two_faces_block", (0.0, Y["two_face"], 0.0), X, light(8.0))
    s.add("equal_t", (0.0, Y["equal_t"], 0.0), X, light(8.0))
    if anyhit:
        s.add("face_at_tlight", (0.0, Y["tie"], 0.0), X, 2.0)
        s.add("face_at_tlight_up", (0.0, Y["tie"], 0.0), X, up(2.0))
        s.add("face_at_tlight_down", (0.0, Y["tie"], 0.0), X, down(2.0))
        s.add("tlight_zero", (0.0, Y["tie"], 0.0), X, 0.0)
        s.add("tlight_below_eps", (0.0, Y["tie"], 0.0), X, 5e-6)
        s.add("tlight_inf", (0.0, Y["tie"], 0.0), X, np.inf)
        s.add("box_beyond_light", (0.0, Y["far_box"], 0.0), X, 4.0)
        if lights:
            s.add("orb_then_front", (0.0, Y["orb_front"], 0.0), X, 5.0)
            s.add("orb_then_behind", (0.0, Y["orb_behind"], 0.0), X, 5.0)
            s.add("orb_tie", (0.0, Y["orb_behind"], 0.0), X, ORB_NEAR)
            s.add("orb_tie_up", (0.0, Y["orb_behind"], 0.0), X, up(ORB_NEAR))
            s.add("orb_tie_down", (0.0, Y["orb_behind"], 0.0), X, down(ORB_NEAR))
    else:
        s.add("t0_at_tnear", (0.0, Y["cull"], 0.0), X, 2.0)
        s.add("t0_at_tnear_up", (0.0, Y["cull"], 0.0), X, up(2.0))
        s.add("t0_at_tnear_down", (0.0, Y["cull"], 0.0), X, down(2.0))
        s.add("hit_at_later_tnear", (0.0, Y["after_hit"], 0.0), X, np.inf)
        s.add("box_beyond_light", (0.0, Y["far_box"], 0.0), X, 4.0)
        if lights:
            s.add("orb_then_front", (0.0, Y["orb_front"], 0.0), X, np.inf)
    return s.done()


CHAIN_PAIRS, CHAIN_END = 300, 400.0


def chain_scene(pbr):
    key = ("walk_rays.chain",)
    if key not in hand_scenes._cache:
        spec = hand_scenes.tree("chain300")
        bvh, faces = hand_scenes.nodes_of(spec)
        tris, leaf = [], 0
        for i, (kind, arg) in enumerate(spec):
            lo, hi = [0.0, -1.0, -1.0], [CHAIN_END, 9.0, 3.0]
            if kind == "l":
                lo[0] = float(leaf)
                for k in range(arg):
                    y = 5.0 + 0.5 * k
                    tris.append([[leaf, y, -1], [leaf, y, 3], [leaf + 1, y, -1]])       # the ray at x = leaf + 1 / 2 meets it at u = 1 / 4, v = 1 / 2
                leaf += 1
            elif i > 0:
                lo[0] = float(leaf)               # the container behind leaf j - 1 holds x >= j
            bvh[i, 0:3], bvh[i, 4:7] = lo, hi
        assert len(tris) == faces and leaf == CHAIN_PAIRS + 2
        tris[0] = [[-256, 7, -1], [-256, 7, 3], [768, 7, -1]]       # leaf 0's one face: behind every other, across the whole chain
        sc = _scene(pbr, bvh, np.array(tris, np.float32), [])
        sc.leaf_faces = np.array([arg for kind, arg in spec if kind == "l"])
        hand_scenes._cache[key] = sc
    return hand_scenes._cache[key]


def chain_ray(i):
    return (i + 0.5, 0.0, 0.0), (0.0, 1.0, 0.0)


def chain_rays(anyhit):
    """Wave 0: lane i leaves after i pairs (a departure in every visit).  Wave 1: one long walk among 63 that miss node 1.
    Wave 2: 64 copies of one ray (every lane parks in the same visit).  Then a blocker in the first leaf and in the last."""
    s = RaySet()
    t0 = 6.0 if anyhit else np.inf
    for i in range(64):
        s.add("departures", *chain_ray(i), t0)
    for i in range(64):
        if i == 37:
            s.add("long_walk", *chain_ray(CHAIN_PAIRS), t0)
        else:
            s.add("miss_node1", (-5.0 - i, 0.0, 0.0), (0.0, 1.0, 0.0), t0)
    for i in range(64):
        s.add("copies", *chain_ray(40), t0)
    s.add("ends_on_last_record", *chain_ray(CHAIN_PAIRS + 1), t0)
    if anyhit:
        for i in (1, 150, CHAIN_PAIRS, CHAIN_PAIRS + 1):
            s.add("blocker_in_first_leaf", *chain_ray(i), 8.0)
            s.add("blocker_in_last_leaf", *chain_ray(i), 6.0)
    return s.done()


def inside_all_rays(sc, anyhit, n=64, seed=3):
    """Rays from the middle of a scene whose boxes are all the scene's (hand_scenes, loose): they start inside every box, so
    tNear < 0 at every node and tFar decides alone.  The any-hit walk's tLight lies among the faces' distances."""
    rng = np.random.default_rng(seed)
    a = sc.arrays
    v = a["vertices"][:, :3].astype(np.float64)
    mid = 0.5 * (v.min(0) + v.max(0)) + rng.uniform(-0.05, 0.05, (n, 3))
    tri = v[a["facesV"][~sc.flat][:, :3].astype(np.int64)]
    target = (tri[rng.integers(0, tri.shape[0], n)] * rng.dirichlet([1.0, 1.0, 1.0], n)[:, :, None]).sum(1)
    direction = np.where((np.arange(n) % 4 == 3)[:, None], rng.normal(size=(n, 3)), target - mid)      # three of four aimed at a face with area
    t_light = rng.uniform(0.25, 2.0, n)
    s = RaySet()
    for o, d, t in zip(mid, hand_scenes._unit(direction), t_light):
        s.add("inside_all", o, d, t if anyhit else np.inf)
    return s.done()


def inside_scene(pbr):
    return hand_scenes.scene(pbr, "wide7", degenerate=True, signed_zeros=True, loose=True)


# ---- random rays and their float64 truth ----------------------------------------------------------------------------------

# the trees the random rays are drawn on: hand trees (the Phong shapes' flat geometry among them) and the generated scene of some
# 2 000 nodes that a staged prefix leaves partly cold
RANDOM_TREES = ("leaf1", "wide7", "wide40", "chain300", "cut257", "ternary10", "generated")
GENERATED = ("hairball", 3, 3000)          # host/scene_gen.cpp: some 2 000 faces under some 2 000 nodes
NATIVE_MARGIN = NATIVE_SCALE * hand_scenes.EDGE_MARGIN      # the boundary clearance at which float64 decides for the native arithmetic
OVERDRAW = 2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_scene(pbr, name):
    if name == "generated":
        key = ("walk_rays.generated",)
        if key not in hand_scenes._cache:
            hand_scenes._cache[key] = refit_scenes.generated(pbr, GENERATED[0], GENERATED[1], GENERATED[2], 32, 24)
        return hand_scenes._cache[key]
    return hand_scenes.scene(pbr, name, degenerate=True, signed_zeros=True)


def random_set(sc, n=2048, seed=7):
    """n ordinary rays at the scene's faces with a random tLight each: for a hit ray uniform in ( 0.2, 1.8 ) times the brute-force
    distance — blocked and lit in equal parts —, for a miss a multiple of the scene's size.  They are not meant to sit on edges:
    OVERDRAW * n candidates are drawn (hand_scenes.rays_at) and those that pass every face's boundary at NATIVE_MARGIN or more
    are kept first, in the order drawn — on a dense lattice (ternary10: 4 600 faces on five points a side) one candidate in six
    does not, and a truth that decides too few rays says little."""
    key = ("walk_rays.random", sc.arrays["vertices"].tobytes(), n, seed)
    if key not in hand_scenes._cache:
        a = sc.arrays
        flat = getattr(sc, "flat", None)
        if flat is None:
            tri = a["vertices"][:, :3][a["facesV"][:, :3].astype(np.int64)].astype(np.float64)
            flat = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) == 0.0
        drawn = hand_scenes.rays_at(a["facesV"], a["vertices"], flat, OVERDRAW * n, seed)
        best, _, _, edge = hand_scenes.brute_force_faces(a["facesV"], a["vertices"], np.asarray(drawn, np.float64))
        clear = edge >= NATIVE_MARGIN
        keep = np.sort(np.concatenate([np.nonzero(clear)[0], np.nonzero(~clear)[0]])[:n])
        rays, best = drawn[keep], best[keep]
        rng = np.random.default_rng(seed + 1)
        size = float(np.linalg.norm(a["vertices"][:, :3].max(0) - a["vertices"][:, :3].min(0)))
        t_light = np.where(np.isfinite(best), best * rng.uniform(0.2, 1.8, n), size * rng.uniform(0.5, 4.0, n)).astype(np.float32)
        hand_scenes._cache[key] = (np.ascontiguousarray(rays), t_light)
    return hand_scenes._cache[key]


def shadow_truth64(sc, rays, t_light, margin=hand_scenes.EDGE_MARGIN):
    """From the inputs alone, in float64 over ALL faces: (decided, blocked, t, edge).  decided: the ray passes every face's boundary at
    `margin` or more, meets no face within wt.T_GUARD of its origin, and is either lit — no accepted hit up to tLight +
    T_GUARD — or blocked — the closest accepted hit lies in ( T_GUARD, tLight - T_GUARD )."""
    a = sc.arrays
    r64 = np.asarray(rays, np.float64)
    tl = np.asarray(t_light, np.float64)
    t, face, gap, edge = hand_scenes.brute_force_faces(a["facesV"], a["vertices"], r64)
    blocked = np.isfinite(t) & (t > wt.T_GUARD) & (t < tl - wt.T_GUARD)
    lit = ~np.isfinite(t) | (t > tl + wt.T_GUARD)
    skip = np.full(r64.shape[0], -1, np.int64)
    at_origin = wt._met_at_the_ends(sc, r64, skip, np.full(r64.shape[0], np.inf))
    return (edge >= margin) & ~at_origin & (blocked | lit), blocked, t, edge
