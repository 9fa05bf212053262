"""Complete scenes under a tree of the caller's choosing (numpy only): the trees no builder makes — a root with one child,
containers of 7 and 40 leaves, chains of height 301 and 1401, trees of 255 / 256 / 257 nodes around the refit's cut, a tree
whose every container has a leaf between two containers — in the flat wire format, with faces, normals, materials, lights,
camera and config, as a refit_scenes.Scene.

A tree is a list in depth-first order of ("c", link) — a container and its miss link — and ("l", faces) — a leaf of 1 or 2
faces.  Faces are numbered in leaf order; every face is one triangle with three vertices of its own.  Triangle centres lie on
a small integer lattice and the corners a multiple of 1/4 away, so many sibling keys tie and both child orders occur.
"""
import numpy as np

import patch_refit_ref
import refit_ref
import refit_scenes

ALPHA = 0.6        # the phong_tessellation of the Phong cases
SHAPES =("leaf1", "leaf2", "wide7", "wide40", "chain300", "chain1400", "cut255", "cut256", "cut257", "ternary10")
# name: (nodes, height of node 0, leaves) — what the shapes are there for, checked by tests/test_hand_scenes_cpu.py
EXPECT = {"leaf1": (2, 1, 1), "leaf2": (2, 1, 1), "wide7": (9, 2, 7), "wide40": (42, 2, 40), "chain300": (603, 301, 302),
          "chain1400": (2803, 1401, 1402), "cut255": (255, 7, 128), "cut256": (256, 7, 129), "cut257": (257, 8, 129),
          "ternary10": (5118, 11, 3071)}
PHONG_SHAPES = ("leaf2", "wide7", "cut257", "ternary10")
WIDTH, HEIGHT, FRAMES, DEPTH, RAYS = 32, 24, 2, 3, 2048
SEED = 11          # of the geometry and of the rays: tests/test_hand_scenes_cpu.py holds the zero-outlier condition for it


# ---- trees ------------------------------------------------------------------------------------------------------------

def _sized(tree):
    """A nested tree — an int is a leaf of that many faces, a list a container of its items — as [("c", subtree size) |
    ("l", faces)] in depth-first order."""
    if isinstance(tree, int):
        return [("l", tree)]
    body = [item for child in tree for item in _sized(child)]
    return [("c", len(body) + 1)] + body


def _linked(sized):
    """Subtree sizes -> miss links: where the subtree ends, -1 when that is the end of the array (the walk stops there)."""
    n = len(sized)
    return [(kind, arg if kind == "l" else (i + arg if i + arg < n else -1)) for i, (kind, arg) in enumerate(sized)]


def _balanced(leaves):
    return 2 if leaves == 1 else [_balanced(leaves - leaves // 2), _balanced(leaves // 2)]


def _ternary(depth):
    return [1, 2] if depth == 0 else [_ternary(depth - 1), 1 + depth % 2, _ternary(depth - 1)]


def _chain(pairs):
    """test_relink_cpu's CHAIN: node 0, then a leaf and a container per level, two leaves at the bottom."""
    n = 3 + 2 * pairs
    sized = [("c", n)]
    for j in range(pairs):
        sized += [("l", 1 + j % 2), ("c", n - (2 + 2 * j))]
    return sized + [("l", 1), ("l", 2)]


def tree(shape):
    if shape in ("leaf1", "leaf2"):
        return _linked(_sized([int(shape[4:])]))
    if shape.startswith("wide"):
        return _linked(_sized([[1 + j % 2 for j in range(int(shape[4:]))]]))
    if shape.startswith("chain"):
        return _linked(_chain(int(shape[5:])))
    if shape == "cut255":
        return _linked(_sized(_balanced(128)))
    if shape == "cut256":
        return _linked(_sized([_balanced(43), _balanced(43), _balanced(43)]))       # 1 + 3 * 85
    if shape == "cut257":
        return _linked(_sized(_balanced(129)))
    if shape == "ternary10":
        return _linked(_sized(_ternary(10)))
    raise ValueError(shape)


def nodes_of(spec):
    """The wire format's .w words of a tree, (N, 8) float32 with every box zero, and its number of faces."""
    bvh = np.zeros((len(spec), 8), np.float32)
    face = 0
    for i, (kind, arg) in enumerate(spec):
        if kind == "c":
            bvh[i, 3], bvh[i, 7] = -1, arg
        else:
            assert arg in (1, 2)
            bvh[i, 3], bvh[i, 7] = face, (face + 1 if arg == 2 else -1)
            face += arg
    return bvh, face


# ---- geometry ---------------------------------------------------------------------------------------------------------

def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def geometry(faces, seed, degenerate=False, signed_zeros=False, phong=False):
    """(facesV, facesN, vertices, normals, flat): face f has vertices and normals 3 f .. 3 f + 2; flat[f]: it has no area.
    degenerate: about an eighth of the faces (never face 0) have three equal corners.  signed_zeros: about a quarter of the
    faces (always the first four) lie in a coordinate plane through 0, the three zeros signed at random — +0 before -0 and
    -0 before +0 both occur.  phong: the last face has three equal normals, the last but one three corners on a line."""
    rng = np.random.default_rng(seed)
    reach = 0 if faces <= 4 else 1 if faces <= 64 else 2     # few faces stay together, so that a camera sees more than sky
    centre = rng.integers(-reach, reach + 1, (faces, 1, 3)).astype(np.float64)
    corners = centre + rng.integers(-4, 5, (faces, 3, 3)) / 4.0
    corners[0] = centre[0] + np.array([[-3, -2, 1], [3, -1, -2], [0, 3, 2]]) / 4.0     # face 0 has area, in every coordinate plane too
    flat = np.zeros(faces, bool)
    if degenerate:
        flat = rng.random(faces) < 0.125
        flat[0] = False
        corners[flat] = corners[flat][:, :1]
    if phong and faces >= 2:
        a, d = corners[faces - 2, 0], np.array([0.25, 0.125, -0.125])
        corners[faces - 2] = [a, a + d, a + 2 * d]
        flat[faces - 2] = True
    corners = corners.astype(np.float32)
    if signed_zeros:
        chosen = rng.random(faces) < 0.25
        chosen[0] = True
        axis = rng.integers(0, 3, faces)
        zeros = np.where(rng.random((faces, 3)) < 0.5, np.float32(-0.0), np.float32(0.0))
        # the first four faces lie in one plane, so that whichever of them share a leaf, its box there is the zero met first
        chosen[:4], axis[:4] = True, axis[0]
        zeros[:4] = [[0.0, -0.0, 0.0], [0.0, 0.0, -0.0], [-0.0, 0.0, -0.0], [-0.0, -0.0, 0.0]][:min(faces, 4)]
        for f in np.nonzero(chosen)[0]:
            corners[f, :, axis[f]] = zeros[f]
    edges = corners.astype(np.float64)
    area = np.cross(edges[:, 1] - edges[:, 0], edges[:, 2] - edges[:, 0])
    flat |= np.linalg.norm(area, axis=1) == 0.0
    # vertex normals: the face's, leaning a seeded way at every corner; a face without area gets any unit vectors
    face_n = np.where(flat[:, None], rng.normal(size=(faces, 3)), area)
    face_n = _unit(np.where(np.linalg.norm(face_n, axis=1, keepdims=True) > 0, face_n, [0.0, 1.0, 0.0]))
    normals = _unit(face_n[:, None, :] + 0.3 * rng.uniform(-1, 1, (faces, 3, 3)))
    if phong:
        normals[faces - 1] = face_n[faces - 1]
    vertices, vnormals = np.zeros((3 * faces, 4), np.float32), np.zeros((3 * faces, 4), np.float32)
    vertices[:, :3], vnormals[:, :3] = corners.reshape(-1, 3), normals.reshape(-1, 3).astype(np.float32)
    facesV = np.zeros((faces, 4), np.uint32)
    facesV[:, :3] = np.arange(3 * faces).reshape(faces, 3)
    return facesV, facesV.copy(), vertices, vnormals, flat


def loose_boxes(bvh, vertices):
    """hand_tree's boxes: every node's is the whole scene's, so all keys are equal and every ray visits every node."""
    out = np.array(bvh, np.float32)
    out[:, 0:3], out[:, 4:7] = vertices[:, :3].min(0), vertices[:, :3].max(0)
    return out


MATERIALS = {1: [[1, 1, 8, 8, 0.08, 0.9, 0, 0, 0.62, 0.58, 0.5, 0, 1, 1, 1, 0]],       # Shirley-Ashikhmin: d, Ni, nu, nv, Rs, Rd
             0: [[1, 1, 1, 0.8, 0.62, 0.58, 0.5, 0, 1, 1, 1, 0]]}                       # Schlick: d, Ni, p, rough
LIGHTS = [[0.5, 4.5, 1.0, 0, 4.0, 3.5, 3.0, 0, 2, 0.4, 0, 0],                           # an orb above the lattice, a point beside it:
          [-2.5, 1.0, 4.25, 0, 1, 1, 1, 0, 1, 0, 0, 0]]                                  # test_gpu_walk_order's cornell_lights at this scale


def make(pbr, shape, seed=SEED, brdf=1, lights=False, degenerate=False, signed_zeros=False, loose=False, phong=False):
    """The scene of a shape as a refit_scenes.Scene; .flat marks its faces without area.  Boxes are refit_ref.refit's (under
    phong: the caller's business — patch_refit_ref.refit needs an alpha), or the whole scene's."""
    bvh, faces = nodes_of(tree(shape))
    facesV, facesN, vertices, normals, flat = geometry(faces, seed, degenerate, signed_zeros, phong)
    bvh = loose_boxes(bvh, vertices) if loose else refit_ref.refit(bvh, facesV, vertices)
    arrays = {"bvh": bvh, "facesV": facesV, "facesN": facesN, "vertices": vertices, "normals": normals,
              "materials": np.array(MATERIALS[brdf], np.float32),
              "lights": np.array(LIGHTS, np.float32) if lights else np.zeros((0, 12), np.float32)}
    cfg = pbr.Config()
    cfg.width, cfg.height, cfg.brdf, cfg.shadow_rays = WIDTH, HEIGHT, brdf, 0
    cfg.max_depth, cfg.max_added_depth, cfg.samples = DEPTH, 0, 1
    cfg.anti_aliasing, cfg.phong_tessellation = 0.0, 0.0
    cfg.sky_light[0], cfg.sky_light[1], cfg.sky_light[2], cfg.sky_light[3] = 0.75, 0.5, 0.25, 0.0
    cfg.tile_world, cfg.tile_rank = 1, 0
    sc = refit_scenes.Scene(pbr, arrays, cfg, camera(pbr, vertices, flat), pbr.pixel_dimension(WIDTH, HEIGHT), pbr.frame_seeds(0, FRAMES))
    sc.flat, sc.shape = flat, shape
    return sc


def camera(pbr, vertices, flat, toward=(4.0, 3.0, 6.0), distance=1.3):
    """A pbr_camera whose view the faces with area fill, however few they are: rays leave the eye along w (+ u and v across
    the image), the basis the host driver derives from eye, centre and up = y; no focus point.  toward, distance: where the
    eye stands, seen from the middle of the faces, in units of their extent."""
    seen = vertices[np.repeat(~flat, 3), :3].astype(np.float64)
    middle, size = 0.5 * (seen.min(0) + seen.max(0)), max(float(np.linalg.norm(seen.max(0) - seen.min(0))), 1.5)
    eye = middle + distance * size * _unit(np.array(toward, np.float64))        # (4, 3, 6): no coordinate plane is seen edge-on
    w = _unit(middle - eye)
    u = _unit(np.cross(w, [0.0, 1.0, 0.0]))
    v = _unit(np.cross(u, w))
    cam = pbr.Camera()
    origin, ahead = np.zeros(3, np.float32), np.array([0, 0, 1], np.float32)
    pbr.host.pbrh_camera_lookat(ahead.ctypes.data_as(pbr._fp), origin.ctypes.data_as(pbr._fp), cam)     # the lense's defaults
    for field, value in (("eye", eye), ("w", w), ("u", u), ("v", v)):
        q = getattr(cam, field)
        q.x, q.y, q.z, q.w = float(value[0]), float(value[1]), float(value[2]), 0.0
    cam.focusPoint[0], cam.focusPoint[1] = -1, -1
    return cam


def with_arrays(sc, **arrays):
    a = dict(sc.arrays)
    a.update({k: np.ascontiguousarray(v, np.float32) for k, v in arrays.items()})
    out = refit_scenes.Scene(sc.pbr, a, sc.cfg, sc.cam, sc.px, sc.seeds)
    out.flat, out.shape = sc.flat, sc.shape
    return out


def move(sc, seed=1):
    """V': every face shifted as a whole by a seeded multiple of 1/8 per axis — a face of three equal corners keeps them
    equal — but not along an axis on which its three corners are zeros: a face in a coordinate plane stays there, signs and all."""
    v = sc.arrays["vertices"]
    rng = np.random.default_rng(seed)
    shift = np.repeat(rng.integers(-6, 7, (v.shape[0] // 3, 3)) / 8.0, 3, axis=0).astype(np.float32)
    in_plane = np.repeat((v[:, :3].reshape(-1, 3, 3) == 0).all(axis=1), 3, axis=0)      # per face and axis: all three corners are zeros
    out = v.copy()
    out[:, :3] = np.where(in_plane, v[:, :3], v[:, :3] + shift)
    return out


def turned_normals(sc, seed=1):
    """N': every vertex normal leaning another seeded way; equal normals of a face stay equal."""
    n = sc.arrays["normals"]
    rng = np.random.default_rng(seed)
    per_corner = n[:, :3].reshape(-1, 3, 3)
    equal = (per_corner == per_corner[:, :1]).all(axis=(1, 2))
    lean = np.where(equal[:, None, None], rng.uniform(-0.2, 0.2, (equal.size, 1, 3)), rng.uniform(-0.2, 0.2, (equal.size, 3, 3)))
    out = n.copy()
    out[:, :3] = _unit(n[:, :3].astype(np.float64) + lean.reshape(-1, 3)).astype(np.float32)
    return out


# ---- rays and the brute force -------------------------------------------------------------------------------------------

def rays_at(facesV, vertices, flat, n=RAYS, seed=SEED):
    """n rays, (n, 6) float32: seven of eight aimed at a random barycentric point of a random face with area, from origins
    on a shell around the scene; the others from there in any direction."""
    rng = np.random.default_rng(seed)
    v = vertices[:, :3].astype(np.float64)
    tri = v[facesV[~flat][:, :3].astype(np.int64)]
    pick = tri[rng.integers(0, tri.shape[0], n)]
    b = rng.dirichlet([1.0, 1.0, 1.0], n)
    target = (pick * b[:, :, None]).sum(1)
    mid, radius = 0.5 * (v.min(0) + v.max(0)), 0.5 * np.linalg.norm(v.max(0) - v.min(0)) + 1.0
    origin = mid + _unit(rng.normal(size=(n, 3))) * rng.uniform(1.0, 2.0, (n, 1)) * radius
    direction = np.where((np.arange(n) % 8 == 7)[:, None], rng.normal(size=(n, 3)), target - origin)
    return np.concatenate([origin, _unit(direction)], axis=1).astype(np.float32)


def brute_force(facesV, vertices, rays):
    """The closest hit of every ray over ALL faces, Moeller-Trumbore in float64 with the acceptance of
    test_gpu_known_answers.test_closest_hits_against_brute_force_in_float64: t, (n,) float64, inf for a miss."""
    tri = vertices[:, :3][facesV[:, :3].astype(np.int64)].astype(np.float64)
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    best = np.full(rays.shape[0], np.inf)
    for k in range(0, rays.shape[0], 64):                      # 64 rays x all faces at a time
        o, dd = rays[k:k + 64, None, 0:3].astype(np.float64), rays[k:k + 64, None, 3:6].astype(np.float64)
        p = np.cross(dd, e2)
        det = (e1 * p).sum(2)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = o - a
            u = (tv * p).sum(2) * inv
            q = np.cross(tv, e1)
            vv = (q * dd).sum(2) * inv
            tt = (e2 * q).sum(2) * inv
            ok = (u >= -1e-6) & (vv >= -1e-6) & (u + vv <= 1 + 1e-6) & (tt > 1e-4) & np.isfinite(tt)
        best[k:k + 64] = np.where(ok, tt, np.inf).min(1)
    return best


def brute_force_faces(facesV, vertices, rays):
    """brute_force() with what it leaves out -> (t, face, gap, edge), each (n,): the closest hit and its face (-1: miss); the
    distance in t to the runner-up among the accepted hits (inf if there is none); and how close, in barycentric units, the
    ray passes to the boundary of ANY face whose plane it meets in front of the origin — an edge of the face it hits, or the
    silhouette of one it just misses.  rays: (n, 6), taken to float64 as they are."""
    tri = vertices[:, :3][facesV[:, :3].astype(np.int64)].astype(np.float64)
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    n = rays.shape[0]
    best, face, gap, edge = np.full(n, np.inf), np.full(n, -1, np.int64), np.full(n, np.inf), np.full(n, np.inf)
    for k in range(0, n, 64):
        o, dd = np.asarray(rays[k:k + 64, None, 0:3], np.float64), np.asarray(rays[k:k + 64, None, 3:6], np.float64)
        p = np.cross(dd, e2)
        det = (e1 * p).sum(2)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = o - a
            u = (tv * p).sum(2) * inv
            q = np.cross(tv, e1)
            vv = (q * dd).sum(2) * inv
            tt = (e2 * q).sum(2) * inv
            ok = (u >= -1e-6) & (vv >= -1e-6) & (u + vv <= 1 + 1e-6) & (tt > 1e-4) & np.isfinite(tt)
            ahead = (tt > 0) & np.isfinite(tt)
            boundary = np.abs(np.minimum(np.minimum(u, vv), 1.0 - (u + vv)))
        hits = np.sort(np.where(ok, tt, np.inf), axis=1)
        best[k:k + 64] = hits[:, 0]
        face[k:k + 64] = np.where(np.isfinite(hits[:, 0]), np.where(ok, tt, np.inf).argmin(1), -1)
        if hits.shape[1] > 1:
            with np.errstate(invalid="ignore"):
                gap[k:k + 64] = np.where(np.isfinite(hits[:, 1]), hits[:, 1] - hits[:, 0], np.inf)
        edge[k:k + 64] = np.where(ahead, boundary, np.inf).min(1)
        edge_on = (np.abs(det) < 1e-12) & (np.linalg.norm(np.cross(e1, e2), axis=1) > 0)
        edge[k:k + 64] = np.where(edge_on.any(1), 0.0, edge[k:k + 64])                    # a face with area seen edge-on is all boundary
    return best, face, gap, edge


def outliers(t, best):
    """The rays outside that test's tolerance, 1e-3 max( 1, t ); a ray that misses in both is inside."""
    t, best = np.asarray(t, np.float64), np.asarray(best, np.float64)
    with np.errstate(invalid="ignore"):
        inside = np.where(np.isinf(t) & np.isinf(best), t == best, np.abs(t - best) <= 1e-3 * np.maximum(1.0, best))
    return np.nonzero(~inside)[0]


# ---- the cases the GPU tests run, established on the CPU first ----------------------------------------------------------

_cache = {}


def scene(pbr, shape, **options):
    """make(), once per case and shared; nobody writes to the arrays."""
    key = (shape,) + tuple(sorted(options.items()))
    if key not in _cache:
        _cache[key] = make(pbr, shape, **options)
    return _cache[key]


def walk_scenes(pbr, shape):
    """(what, scene) of the walk tests: zeros of both signs and faces of three equal corners, under tight and under loose boxes."""
    yield "tight", scene(pbr, shape, degenerate=True, signed_zeros=True)
    yield "loose", scene(pbr, shape, degenerate=True, signed_zeros=True, loose=True)


def rays_of(sc, seed=SEED):
    """The rays of a scene's geometry (the same under tight and loose boxes), once."""
    key = ("rays", sc.arrays["vertices"].tobytes(), seed)
    if key not in _cache:
        _cache[key] = rays_at(sc.arrays["facesV"], sc.arrays["vertices"], sc.flat, RAYS, seed)
    return _cache[key]


def brute_force_of(sc, seed=SEED):
    key = ("brute", sc.arrays["vertices"].tobytes(), seed)
    if key not in _cache:
        _cache[key] = brute_force(sc.arrays["facesV"], sc.arrays["vertices"], rays_of(sc, seed))
    return _cache[key]


def phong_case(pbr, shape, seed=1):
    """(S, V', N', S') under Phong tessellation ALPHA: distinct vertex normals, one face with equal normals, one without
    area; the moved scene has patch_refit_ref's thick boxes."""
    key = ("phong", shape, seed)
    if key not in _cache:
        sc = scene(pbr, shape, phong=True)
        a = sc.arrays
        v, n = move(sc, seed), turned_normals(sc, seed)
        nodes = patch_refit_ref.refit(a["bvh"], a["facesV"], a["facesN"], v, n, ALPHA)
        _cache[key] = (sc, v, n, with_arrays(sc, vertices=v, normals=n, bvh=nodes))
    return _cache[key]


def moved(sc, seed=1):
    """(V', S'): sc's vertices moved and the scene a fresh upload would take, refit_ref.refit's boxes."""
    key = ("moved", id(sc), seed)
    if key not in _cache:
        v = move(sc, seed)
        _cache[key] = (sc, v, with_arrays(sc, vertices=v, bvh=refit_ref.refit(sc.arrays["bvh"], sc.arrays["facesV"], v)))
    return _cache[key][1:]


# ---- the feature pass: every pixel-centre ray of a camera, far from every edge -------------------------------------------------

FEATURE_W, FEATURE_H = 64, 48
FEATURE_KD = [[0.62, 0.58, 0.5], [0.1, 0.6, 0.2], [0.9, 0.15, 0.1]]      # face f has material f % 3
EDGE_MARGIN = 1e-5       # barycentric: ten times brute_force's own acceptance band, which is what a binary32 ray can move a hit by
# shape: (toward, distance) of camera() — found by trying a few eyes; tests/test_filter_planes_cpu.py holds what they are there for
FEATURE_CAMERAS = {"wide7": ((5.0, 2.0, 4.0), 0.5), "wide40": ((6.0, 1.0, 3.0), 0.9)}


def centre_rays64(cam, px, w, h):
    """The rays through the pixel centres (pathtracing.cl:25-48 without jitter and lens) in float64 from the camera's binary32
    fields and the binary32 pixel dimension: (h * w, 6), row-major, row 0 = bottom."""
    eye, cw, cu, cv = (np.array([q.x, q.y, q.z], np.float64) for q in (cam.eye, cam.w, cam.u, cam.v))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    inner = (cu - cu * w) + cu * (2.0 * xs[..., None]) + cv - cv * h + cv * (2.0 * ys[..., None])
    direction = _unit(cw + inner * (float(np.float32(px)) * 0.5))
    return np.concatenate([np.broadcast_to(eye, direction.shape), direction], axis=-1).reshape(-1, 6)


def feature_case(pbr, shape):
    """A scene of `shape` with three materials, flat faces and no lights at FEATURE_W x FEATURE_H under FEATURE_CAMERAS[shape]
    -> (scene, rays64 (h * w, 6), brute_force_faces of them)."""
    key = ("features", shape)
    if key not in _cache:
        base = scene(pbr, shape)
        a = dict(base.arrays)
        a["facesV"] = a["facesV"].copy()
        a["facesV"][:, 3] = np.arange(a["facesV"].shape[0]) % len(FEATURE_KD)
        a["facesN"] = a["facesV"].copy()
        a["materials"] = np.repeat(np.array(MATERIALS[1], np.float32), len(FEATURE_KD), axis=0)
        a["materials"][:, 8:11] = FEATURE_KD
        toward, distance = FEATURE_CAMERAS[shape]
        cam = camera(pbr, a["vertices"], base.flat, toward, distance)
        sc = refit_scenes.Scene(pbr, a, base.config(width=FEATURE_W, height=FEATURE_H), cam, pbr.pixel_dimension(FEATURE_W, FEATURE_H), base.seeds)
        sc.flat, sc.shape = base.flat, shape
        rays = centre_rays64(cam, sc.px, FEATURE_W, FEATURE_H)
        _cache[key] = (sc, rays, brute_force_faces(a["facesV"], a["vertices"], rays))
    return _cache[key]
