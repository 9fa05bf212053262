"""Known answers the render calls themselves give about the walk, per pixel (numpy only, no device): two configurations in
which an image is a readout of the closest-hit walk and of the any-hit walk, and their truth from a float64 brute force over
all faces — no tree, no oracle.

With anti_aliasing = 0 the jitter of a camera ray is multiplied by 0: every frame's ray is the pixel-centre ray
(hand_scenes.centre_rays64).  With samples = 1, max_added_depth = 0, no focus point and one matte material of d = 1 that never
extends a path (MATERIALS: nu, nv < 50; rough = 1), pathtracing.cl:251-334 leaves

  A  max_depth = 1, sky (0.75, 0.5, 0.25), no lights, shadow_rays = 0:  .w = the first hit's ray.t (:261) or inf; a path that
     hits ends at :274 without contribution, rgb exactly 0; a path that misses takes the sky, exactly.
  B  max_depth = 2, sky 0, shadow_rays = 1, one point light:  at depth 0 a hit runs shadowRayTest (:188-199) through
     traverseShadows and adds the direct term only if nothing blocks and |pdf| > 1e-5 (:104-116 / :135-156); depth 1 either
     misses — times the black sky — or ends at :274 with light.x = -1.  rgb != 0 exactly where the any-hit walk found the
     light visible and the BRDF gate passed.

A pixel is a known answer only where the inputs decide it: far from every edge and silhouette in barycentric units (`edge`
of hand_scenes.brute_force_faces), not grazing (barycentric error grows as 1 / cosine), and, for the shadow ray that leaves a
binary32 hit point, not grazing the hit face either (the self-hit guard t < EPSILON5 of pt_intersect.cl:107) and with no
other face within 1e-3 of either end.  These masks are functions of the inputs alone.
"""
import numpy as np

import hand_scenes
import refit_ref
import refit_scenes
import shading_ref

COSINE_MIN = 0.05            # of the camera ray on the face it hits
LIGHT_COSINE_MIN = 0.1       # of the light ray on the face it leaves
T_GUARD = 1e-3               # a blocker counts between T_GUARD and tLight - T_GUARD; nothing else may be met at either end
LIT_FLOOR = 2.0 ** -10       # of the predicted direct term's largest channel: far above any rounding of either arithmetic
SKY = (0.75, 0.5, 0.25)
LIGHT_RGB = (4.0, 3.5, 3.0)
W, H, FRAMES = hand_scenes.FEATURE_W, hand_scenes.FEATURE_H, 2
DEFECTS = ("second_face", "shrunk_box", "skipped_subtree")
# matte, d = 1, never extending a path (pt_utils.cl:89-96): hand_scenes.MATERIALS, but the Schlick one with rough = 1 — at its
# 0.8 a fifth of the paths draw addDepth, go on past max_depth's last hit and shade there
MATERIALS = {1: hand_scenes.MATERIALS[1], 0: [hand_scenes.MATERIALS[0][0][:3] + [1.0] + hand_scenes.MATERIALS[0][0][4:]]}


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def triangles64(sc):
    a = sc.arrays
    return a["vertices"][:, :3][a["facesV"][:, :3].astype(np.int64)].astype(np.float64)


def face_normals64(sc):
    """fast_normalize( cross( edge1, edge2 ) ) of pt_intersect.cl:122 in float64: the unflipped geometric normal; NaN without area."""
    tri = triangles64(sc)
    with np.errstate(invalid="ignore", divide="ignore"):
        return _unit(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]))


# ---- the truth ------------------------------------------------------------------------------------------------------------

def first_hit_truth(sc, w=W, h=H):
    """The pixel-centre rays of sc's camera against all faces in float64 -> {rays (n, 6), t, face, gap, edge, hit, normal (n, 3)
    of the hit face, cosine = |d . n_face| (inf on a miss: nothing grazes)}, row-major, row 0 = bottom."""
    rays = hand_scenes.centre_rays64(sc.cam, sc.px, w, h)
    t, face, gap, edge = hand_scenes.brute_force_faces(sc.arrays["facesV"], sc.arrays["vertices"], rays)
    hit = face >= 0
    normal = np.where(hit[:, None], face_normals64(sc)[np.maximum(face, 0)], 0.0)
    cosine = np.where(hit, np.abs((rays[:, 3:6] * normal).sum(1)), np.inf)
    return {"rays": rays, "t": t, "face": face, "gap": gap, "edge": edge, "hit": hit, "normal": normal, "cosine": cosine}


def decided(edge, cosine, margin):
    """Input-only: the ray passes every boundary at `margin` or more and does not graze what it hits (cosine = inf on a miss)."""
    return (edge >= margin) & (cosine >= COSINE_MIN)


def _met_at_the_ends(sc, rays, skip, t_light):
    """Per ray: some face other than skip[ray] is met — inside brute_force's own acceptance band — at |t| <= T_GUARD or within
    T_GUARD of t_light.  A binary32 origin may lie that far to either side of the float64 one, so t < 0 counts."""
    tri = triangles64(sc)
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    out = np.zeros(rays.shape[0], bool)
    faces = np.arange(tri.shape[0])
    for k in range(0, rays.shape[0], 64):
        o, dd = rays[k:k + 64, None, 0:3], rays[k:k + 64, None, 3:6]
        p = np.cross(dd, e2)
        det = (e1 * p).sum(2)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = o - a
            u = (tv * p).sum(2) * inv
            q = np.cross(tv, e1)
            vv = (q * dd).sum(2) * inv
            tt = (e2 * q).sum(2) * inv
            inside = (u >= -1e-6) & (vv >= -1e-6) & (u + vv <= 1 + 1e-6) & np.isfinite(tt)
            near = (np.abs(tt) <= T_GUARD) | (np.abs(tt - t_light[k:k + 64, None]) <= T_GUARD)
        out[k:k + 64] = (inside & near & (faces[None, :] != skip[k:k + 64, None])).any(1)
    return out


def shadow_truth(sc, light_pos, first):
    """The shadow ray of every hit pixel, from the float64 hit point P = o + t64 d towards the light, against all faces but
    the one it leaves -> per pixel {P, L (unit), t_light, occluded, visible, blocker (the closest one's face, -1), sole (it
    is the only face in front of the light), edge, light_cosine = |L . n_face|, clear (no other face met at either end)};
    everything False / inf on a miss pixel.  occluded: an accepted hit with T_GUARD < t < t_light - T_GUARD; visible: no
    accepted hit at all in front of the light (brute_force_faces knows no far end: what lies more than T_GUARD behind the
    light is no hit of a shadow ray, pt_bvh.cl:17 with ray.t = tLight).

    The face it leaves needs no removing: from P it lies at t = 0, outside brute_force_faces' acceptance (t > 1e-4) — asserted —
    and in `edge` it can only appear with the first hit's own barycentric margin, which never makes a pixel decided."""
    n = first["t"].shape[0]
    hit = first["hit"]
    rays, t = first["rays"][hit], first["t"][hit]
    P = rays[:, 0:3] + t[:, None] * rays[:, 3:6]
    to_light = np.asarray(light_pos, np.float64)[None, :] - P
    t_light = np.linalg.norm(to_light, axis=1)
    L = to_light / t_light[:, None]
    shadow_rays = np.concatenate([P, L], axis=1)
    a = sc.arrays
    bt, bface, bgap, bedge = hand_scenes.brute_force_faces(a["facesV"], a["vertices"], shadow_rays)
    assert not (bface == first["face"][hit]).any()
    blocked = np.isfinite(bt) & (bt < t_light - T_GUARD)
    beyond = np.isfinite(bt) & ~blocked                                # the closest accepted hit lies at or behind the light
    out = {"P": np.zeros((n, 3)), "L": np.zeros((n, 3)), "t_light": np.full(n, np.inf), "occluded": np.zeros(n, bool),
           "visible": np.zeros(n, bool), "blocker": np.full(n, -1, np.int64), "sole": np.zeros(n, bool),
           "edge": np.full(n, np.inf), "light_cosine": np.zeros(n), "clear": np.zeros(n, bool)}
    out["P"][hit], out["L"][hit], out["t_light"][hit] = P, L, t_light
    out["occluded"][hit] = blocked & (bt > T_GUARD)
    out["visible"][hit] = ~np.isfinite(bt) | (beyond & (bt > t_light + T_GUARD))
    out["blocker"][hit] = np.where(blocked, bface, -1)
    # the only blocker: the runner-up, if any, lies behind the light
    out["sole"][hit] = blocked & ~(np.isfinite(bgap) & (bt + bgap < t_light + T_GUARD))
    out["edge"][hit] = bedge
    out["light_cosine"][hit] = np.abs((L * first["normal"][hit]).sum(1))
    out["clear"][hit] = ~_met_at_the_ends(sc, shadow_rays, first["face"][hit], t_light)
    return out


def shadow_decided(first, shadow, margin):
    """Input-only: the pixel's first hit is decided, and so is its shadow ray's verdict."""
    return (first["hit"] & decided(first["edge"], first["cosine"], margin) & (shadow["edge"] >= margin)
            & (shadow["light_cosine"] >= LIGHT_COSINE_MIN) & shadow["clear"] & (shadow["occluded"] | shadow["visible"]))


def lit_gate(sc, brdf, first, light, K, shadow=None):
    """shading_ref.surface_step( brdf ) in float64 at every hit pixel — ray direction d, the hit face's normal, light direction
    L / tLight, lit = 1, the light's rgb, color = 1 -> {passes: got_light is 1, no decision on the way to it is ambiguous at K
    (shading_ref.Analysis) and the predicted direct term's largest channel is at least LIT_FLOOR; final (n, 3)}.  The draws
    only steer the sampled direction, which neither got_light nor the direct term sees (the "N." and sampler decisions)."""
    shadow = shadow if shadow is not None else shadow_truth(sc, light[0:3], first)
    hit = np.flatnonzero(first["hit"])
    n = first["t"].shape[0]
    out = {"passes": np.zeros(n, bool), "final": np.zeros((n, 3))}
    if hit.size == 0:
        return out
    mtl = shading_ref.f32(sc.arrays["materials"][0])
    x = {"dir": first["rays"][hit, 3:6], "normal": first["normal"][hit], "color": np.ones((hit.size, 3)),
         "lightDir": shadow["L"][hit], "lightRgb": np.broadcast_to(np.asarray(light[4:7], np.float64), (hit.size, 3)).copy(),
         "lit": np.ones(hit.size), "draws": np.full((hit.size, shading_ref.DRAWS), 0.5)}
    keys = (1, 2, 3, 4, 5, 6, 8, 9, 10) if brdf == 0 else (1, 2, 3, 4, 5, 8, 9, 10, 12, 13, 14)
    an = shading_ref.Analysis(shading_ref.surface_step(brdf), mtl, x, keys)
    val = an.res["val"]
    ambiguous = np.zeros(hit.size, bool)
    for key, which in an.ambiguous(K).items():
        if key.startswith("U.") or key.startswith("L."):
            ambiguous |= which
    final = val[:, 6:9]
    with np.errstate(invalid="ignore"):
        bright = np.isfinite(final).all(1) & (final.max(1) >= LIT_FLOOR)
    out["passes"][hit] = (val[:, 9] == 1.0) & ~ambiguous & bright
    out["final"][hit] = final
    return out


def sets(first, shadow, gate, margin):
    """(decided, black, lit): the pixels probe A judges; the pixels probe B holds to exactly 0 — decided occluded ones and
    decided misses; the pixels probe B holds to some channel > 0 — decided visible ones that pass the lit gate."""
    mask = decided(first["edge"], first["cosine"], margin)
    sd = shadow_decided(first, shadow, margin)
    return mask, (sd & shadow["occluded"]) | (mask & ~first["hit"]), sd & shadow["visible"] & gate["passes"]


# ---- the two probes ---------------------------------------------------------------------------------------------------------

def config_a(sc, brdf, **fields):
    cfg = sc.config(width=W, height=H, brdf=brdf, max_depth=1, max_added_depth=0, samples=1, shadow_rays=0, anti_aliasing=0.0,
                    phong_tessellation=0.0, **fields)
    cfg.sky_light[0], cfg.sky_light[1], cfg.sky_light[2], cfg.sky_light[3] = SKY[0], SKY[1], SKY[2], 0.0
    return cfg


def config_b(sc, brdf, **fields):
    cfg = sc.config(width=W, height=H, brdf=brdf, max_depth=2, max_added_depth=0, samples=1, shadow_rays=1, anti_aliasing=0.0,
                    phong_tessellation=0.0, **fields)
    cfg.sky_light[0], cfg.sky_light[1], cfg.sky_light[2], cfg.sky_light[3] = 0.0, 0.0, 0.0, 0.0
    return cfg


def probe_a(image, first, mask):
    """An image of configuration A against the truth -> {outliers: decided pixels whose .w lies outside 1e-3 max( 1, t ) of
    t64 (hand_scenes.outliers), colour: decided pixels whose rgb is not exactly 0 on a hit / the sky on a miss, worst: the
    largest |w - t64| / max( 1, t64 ) over the decided hit pixels that hit in both}."""
    img = np.asarray(image).reshape(-1, 4)
    at = np.flatnonzero(mask)
    w, t = img[at, 3].astype(np.float64), first["t"][at]
    outliers = at[hand_scenes.outliers(w, t)]
    want = np.where(first["hit"][at, None], np.float32(0.0), np.asarray(SKY, np.float32)[None, :])
    colour = at[(img[at, :3] != want).any(1)]
    both = np.isfinite(w) & np.isfinite(t)
    worst = float((np.abs(w[both] - t[both]) / np.maximum(1.0, t[both])).max()) if both.any() else 0.0
    return {"outliers": outliers, "colour": colour, "worst": worst}


def probe_b(image, black, lit):
    """An image of configuration B -> {leaks: pixels of the black set with a channel != 0, dark: pixels of the lit set with no
    channel > 0}."""
    rgb = np.asarray(image).reshape(-1, 4)[:, :3]
    with np.errstate(invalid="ignore"):
        return {"leaks": np.flatnonzero(black & (rgb != 0).any(1)), "dark": np.flatnonzero(lit & ~(rgb > 0).any(1))}


def describe(first, image, pixels, limit=4):
    img = np.asarray(image).reshape(-1, 4)
    return [(int(k), img[k].tolist(), float(first["t"][k]), int(first["face"][k])) for k in pixels[:limit]]


# ---- the cases ----------------------------------------------------------------------------------------------------------

# name: (how the geometry is made, camera( toward, distance ), the point light's position) — eyes and lights found by trying
# a few; tests/test_walk_truth_cpu.py holds the conditions they are there for
CASES = {
    "wide7": (("hand", "wide7", False), hand_scenes.FEATURE_CAMERAS["wide7"], (2.5, -1.0, 0.5)),
    "wide40": (("hand", "wide40", False), hand_scenes.FEATURE_CAMERAS["wide40"], (3.0, 4.0, 3.0)),
    "chain300": (("hand", "chain300", True), ((4.0, 3.0, 6.0), 0.9), (4.0, 6.0, 5.0)),
    "cut257": (("hand", "cut257", False), ((4.0, 3.0, 6.0), 0.9), (4.0, 6.0, 5.0)),
    "cornell": (("generated", "cornell", 1, 0), ((0.0, 0.0, 1.0), 1.2), (0.0, 0.5, 0.0)),
    "sponza-6k": (("generated", "sponza", 6, 6000), ((1.0, -0.4, 0.0), 0.25), (-3.0, 1.0, -1.0)),
}
BRDFS = {"wide7": (1,), "wide40": (1, 0), "chain300": (1,), "cut257": (1,), "cornell": (1, 0), "sponza-6k": (1,)}
_cache = {}


def light_row(position, rgb=LIGHT_RGB):
    """A point light (data.x = 1) in the wire format: pos, rgb, data."""
    return np.array([[position[0], position[1], position[2], 0, rgb[0], rgb[1], rgb[2], 0, 1, 0, 0, 0]], np.float32)


def _geometry(pbr, how):
    """The arrays of a case's geometry and tree, every face of material 0, and the faces without area."""
    if how[0] == "hand":
        base = hand_scenes.scene(pbr, how[1], loose=how[2])
        arrays, flat = dict(base.arrays), base.flat
    else:
        pbr.cfg_reset()
        host = pbr.HostScene.generate(how[1], how[2], how[3])
        got = host.arrays()
        arrays = {k: np.ascontiguousarray(got[k]) for k in refit_scenes.ARRAYS}
        tri = arrays["vertices"][:, :3][arrays["facesV"][:, :3].astype(np.int64)].astype(np.float64)
        flat = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) == 0
    arrays["facesV"] = arrays["facesV"].copy()
    arrays["facesV"][:, 3] = 0
    return arrays, flat


def scene_of(pbr, arrays, brdf, cam, light):
    a = dict(arrays)
    a["materials"] = np.array(MATERIALS[brdf], np.float32)
    a["lights"] = light_row(light)
    cfg = hand_scenes.scene(pbr, "leaf1").config(width=W, height=H, brdf=brdf)
    return refit_scenes.Scene(pbr, a, cfg, cam, pbr.pixel_dimension(W, H), pbr.frame_seeds(0, FRAMES))


def case(pbr, name, brdf=1):
    """The scene of a case under one BRDF's matte material, with the case's camera and its one point light; once, shared."""
    key = ("case", name, brdf)
    if key not in _cache:
        how, (toward, distance), light = CASES[name]
        if ("geometry", name) not in _cache:
            _cache[("geometry", name)] = _geometry(pbr, how)
        arrays, flat = _cache[("geometry", name)]
        corners = arrays["vertices"][arrays["facesV"][:, :3].astype(np.int64).reshape(-1)]      # three per face, as camera() takes them
        cam = hand_scenes.camera(pbr, corners, flat, toward, distance)
        sc = scene_of(pbr, arrays, brdf, cam, light)
        sc.flat, sc.shape, sc.light = flat, name, light_row(light)[0].astype(np.float64)
        _cache[key] = sc
    return _cache[key]


def truth(pbr, name, brdf, K):
    """(scene, first, shadow, gate) of a case, once per (case, BRDF): the geometry's brute force is shared between the BRDFs."""
    key = ("truth", name, brdf)
    if key not in _cache:
        sc = case(pbr, name, brdf)
        if ("rays", name) not in _cache:
            first = first_hit_truth(sc)
            _cache[("rays", name)] = (first, shadow_truth(sc, sc.light[0:3], first))
        first, shadow = _cache[("rays", name)]
        _cache[key] = (sc, first, shadow, lit_gate(sc, brdf, first, sc.light, K, shadow))
    return _cache[key]


# ---- planted defects --------------------------------------------------------------------------------------------------

def _misses_box(rays, lo, hi):
    """The slab test in float64, per ray: the ray passes the box [lo, hi] by."""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / rays[:, 3:6]
        t1, t2 = (lo - rays[:, 0:3]) * inv, (hi - rays[:, 0:3]) * inv
        near, far = np.fmin(t1, t2).max(1), np.fmax(t1, t2).min(1)
    return ~(near <= far) | (far <= 0)


def plant(sc, defect, first=None, mask=None, among=None):
    """A copy of the scene with one planted tree defect -> (scene, what): `what` names the node and the pixels (decided, with
    the runner-up well behind) that the unplanted truth says must change.

      "second_face"      a leaf of two faces loses its second (bbMax.w = -1): one whose second face is the float64 first hit
                         of a decided pixel (and one of `among`, if given);
      "shrunk_box"       a leaf's box pulled in by 2 % of its extent on every side: one that a decided pixel's ray then
                         passes by although its first hit lies in that leaf;
      "skipped_subtree"  a container's miss link copied onto its first child, itself a container: one whose first child's box
                         a decided pixel's ray passes by although its first hit lies behind that child, inside the container.
                         The links still run forward.  ValueError if the tree has no such pair."""
    first = first if first is not None else first_hit_truth(sc)
    mask = mask if mask is not None else decided(first["edge"], first["cosine"], hand_scenes.EDGE_MARGIN)
    bvh = sc.arrays["bvh"].copy()
    leaf, face0, face1, end, parent = refit_ref.tree_tables(bvh)
    clear = mask & first["hit"] & (first["gap"] > 1e-2 * np.maximum(1.0, first["t"]))
    leaf_of = np.full(sc.arrays["facesV"].shape[0], -1, np.int64)
    for i in np.flatnonzero(leaf):
        leaf_of[face0[i]] = i
        if face1[i] >= 0:
            leaf_of[face1[i]] = i
    if defect == "second_face":
        for i in np.flatnonzero(leaf & (face1 >= 0)):
            pixels = np.flatnonzero(clear & (first["face"] == face1[i]))
            if pixels.size and (among is None or face1[i] in among):
                bvh[i, 7] = -1
                return hand_scenes.with_arrays(sc, bvh=bvh), {"node": int(i), "face": int(face1[i]), "pixels": pixels}
    elif defect == "shrunk_box":
        for i in np.flatnonzero(leaf):
            lo, hi = bvh[i, 0:3].astype(np.float64), bvh[i, 4:7].astype(np.float64)
            pull = 0.02 * (hi - lo)
            pixels = np.flatnonzero(clear & (leaf_of[np.maximum(first["face"], 0)] == i))
            pixels = pixels[_misses_box(first["rays"][pixels], lo + pull, hi - pull)] if pixels.size else pixels
            if pixels.size:
                bvh[i, 0:3], bvh[i, 4:7] = (lo + pull).astype(np.float32), (hi - pull).astype(np.float32)
                return hand_scenes.with_arrays(sc, bvh=bvh), {"node": int(i), "pixels": pixels}
    elif defect == "skipped_subtree":
        for i in np.flatnonzero(~leaf):
            k = i + 1
            if k >= bvh.shape[0] or leaf[k] or end[k] == end[i]:
                continue
            behind = (leaf_of[np.maximum(first["face"], 0)] >= end[k]) & (leaf_of[np.maximum(first["face"], 0)] < end[i])
            pixels = np.flatnonzero(clear & behind)
            pixels = pixels[_misses_box(first["rays"][pixels], bvh[k, 0:3].astype(np.float64), bvh[k, 4:7].astype(np.float64))] if pixels.size else pixels
            if pixels.size:
                bvh[k, 7] = bvh[i, 7]
                return hand_scenes.with_arrays(sc, bvh=bvh), {"node": int(k), "pixels": pixels}
    else:
        raise ValueError(defect)
    raise ValueError("no place for %r in %s" % (defect, getattr(sc, "shape", "this scene")))
