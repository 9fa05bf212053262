"""Regenerates tests/golden/refkernel_*.npz (container only: needs the reference's tree; oracle/refkernel.py builds the binaries).

    python tests/golden/make_refkernel.py             every recording
    python tests/golden/make_refkernel.py --walk      refkernel_walk_<case>.npz alone (WALK_CASES below: the two walks per ray)

What is stored is DATA the reference's own compiled KERNEL text produced (oracle/refkernel.py: the OpenCL C assembled as its
host assembles it, built unmodified for the CPU behind this repository's builtin shim and driver): per case

    image, debug      the accumulated image and the last frame's debug image, (H, W, 4) float32
    frame_counts      (frames, 2) uint32: node visits and face tests of each frame, the sums of that frame's debug image
    ray_t, ray_face, ray_normal, ray_counts     the closest hits of the case's ray batch (cases with rays only)
    orb_pixels        cases with lights: how many pixel-centre camera rays end on an orb light (hitFace < 0)
    light_census      cases with lights: [faces hidden from the first light, faces it sees], by rays from the light to every face
    values_keys / values_values     the placeholder texts the binary was compiled with

No input is stored: case_inputs() takes them from the fixtures already committed (ref_*.npz, refhost_*.npz) and from
tests/hand_scenes.py, so the GPU tests need neither the reference nor a binary.  Every case names the code it is there to
reach and how the reference's own output shows that it did (REACH); tests/test_refkernel_cpu.py repeats that on the
recorded data.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from make_reference_scenes import CONFIG_FIELDS          # noqa: E402
from make_refhost import SIZE_CAP                        # noqa: E402

WIRE = ("bvh", "facesV", "facesN", "vertices", "normals", "materials", "lights")
RAYS = 2048
REF_SCENES = ("ref_pillars_sa", "ref_pillars_schlick", "ref_suzanne_sa", "ref_suzanne_schlick", "ref_suzanne_sa_shadow",
              "ref_suzanne_schlick_shadow", "ref_spheres_sa", "ref_spheres_schlick", "ref_applejack2_sa", "ref_applejack3_schlick",
              "ref_squirrel_mirror_sa", "ref_squirrel_mirror_schlick", "ref_squirrels_sa", "ref_squirrels_schlick")

# name: {base: the ref_* fixture whose inputs the case starts from, or hand: (shape, options) of tests/hand_scenes.py;
#        geometry: a refhost_* fixture whose wire arrays replace the base's; set: pbr_config fields; focus: (x, y);
#        first: the first sample count; rays: trace the batch; frames}
CASES = {}
# what each case is there to reach and the evidence: ("equals", fixture) — image, debug and rays equal that committed
# fixture's; ("differs", case) — the image differs from that case's, which is this one with the feature off;
# ("edge",) — box_edge_rays: no face test at tFar <= EPSILON5, at least one from one place above it on;
# ("shadows",) — light_census: the first light sees some faces and is kept from others; ("orb",) — orb_pixels > 0; ("focus", "hit" | "miss") — the focus pixel's .w after the last frame is finite | inf
REACH = {}


def _case(name, reach, **spec):
    CASES[name] = spec
    REACH[name] = reach


for _f in REF_SCENES:       # both BRDFs, plain, every shipped scene — shadow_rays 1 with suzanne.lights among them
    _case("plain_" + _f[4:], [("equals", _f)], base=_f, rays=True)
# shadow rays against the same lights with the shadow rays off (the orb still ends paths: traverseLights)
for _b in ("sa", "schlick"):
    _case("suzanne_%s_lights_noshadow" % _b, [("orb",)], base="ref_suzanne_%s_shadow" % _b, set={"shadow_rays": 0})
    REACH["plain_suzanne_%s_shadow" % _b] += [("differs", "suzanne_%s_lights_noshadow" % _b), ("shadows",), ("orb",)]
# Phong tessellation over the boxes the reference's host grew for that alpha
for _b in ("sa", "schlick"):
    _case("phong06_spheres_" + _b, [("differs", "plain_spheres_" + _b)], base="ref_spheres_" + _b, geometry="refhost_spheres_a0.6",
          set={"phong_tessellation": 0.6}, rays=True)
    _case("phong10_suzanne_" + _b, [("differs", "plain_suzanne_%s_shadow" % _b)], base="ref_suzanne_%s_shadow" % _b,
          geometry="refhost_suzanne_a1.0", set={"phong_tessellation": 1.0}, rays=True)
# SAMPLES > 1: the second and third camera paths of a pixel and the division by SAMPLES
_case("samples2_spheres_sa", [("differs", "plain_spheres_sa")], base="ref_spheres_sa", set={"samples": 2})
_case("samples2_suzanne_schlick", [("differs", "plain_suzanne_schlick")], base="ref_suzanne_schlick", set={"samples": 2})
_case("samples3_pillars_schlick", [("differs", "plain_pillars_schlick")], base="ref_pillars_schlick", set={"samples": 3})
_case("samples3_squirrels_sa", [("differs", "plain_squirrels_sa")], base="ref_squirrels_sa", set={"samples": 3})
# depth of field: the previous frame's .w of the pixel and of the focus pixel; four frames
_case("dof_hit_suzanne_sa", [("differs", "plain4_suzanne_sa"), ("focus", "hit")], base="ref_suzanne_sa", focus=(32, 22), frames=4)
_case("dof_miss_suzanne_sa", [("differs", "plain4_suzanne_sa"), ("differs", "dof_hit_suzanne_sa"), ("focus", "miss")], base="ref_suzanne_sa", focus=(2, 45), frames=4)
_case("dof_hit_spheres_schlick", [("differs", "plain4_spheres_schlick"), ("focus", "hit")], base="ref_spheres_schlick", focus=(20, 30), frames=4)
_case("plain4_suzanne_sa", [], base="ref_suzanne_sa", frames=4)
_case("plain4_spheres_schlick", [], base="ref_spheres_schlick", frames=4)
# one bounce, no extension: the early exit on the last round
_case("depth1_pillars_sa", [("differs", "plain_pillars_sa")], base="ref_pillars_sa", set={"max_depth": 1, "max_added_depth": 0})
_case("depth1_suzanne_schlick", [("differs", "plain_suzanne_schlick")], base="ref_suzanne_schlick", set={"max_depth": 1, "max_added_depth": 0})
# path extension off against the fixtures' 5: suzanne and spheres have nu = nv = 1e5 lobes (Shirley-Ashikhmin extends on
# max( nu, nv ) >= 50), every Schlick material extends where rough < rand()
_case("added0_suzanne_sa", [("differs", "plain_suzanne_sa")], base="ref_suzanne_sa", set={"max_added_depth": 0})
_case("added0_spheres_schlick", [("differs", "plain_spheres_schlick")], base="ref_spheres_schlick", set={"max_added_depth": 0})
# anti-aliasing 0 and 1.5 (the fixtures have 0.7)
_case("aa0_pillars_sa", [("differs", "plain_pillars_sa")], base="ref_pillars_sa", set={"anti_aliasing": 0.0})
_case("aa15_pillars_sa", [("differs", "plain_pillars_sa"), ("differs", "aa0_pillars_sa")], base="ref_pillars_sa", set={"anti_aliasing": 1.5})
_case("aa0_squirrel_mirror_schlick", [("differs", "plain_squirrel_mirror_schlick")], base="ref_squirrel_mirror_schlick", set={"anti_aliasing": 0.0})
_case("aa15_squirrel_mirror_schlick", [("differs", "plain_squirrel_mirror_schlick")], base="ref_squirrel_mirror_schlick", set={"anti_aliasing": 1.5})
# accumulation that starts at sample count 5: the weights 5/6, 6/7, 7/8 over an empty image
_case("first5_spheres_sa", [("differs", "plain_spheres_sa")], base="ref_spheres_sa", first=5)
# hand-made trees with zeros of both signs and faces without area: 2 nodes, and a chain of some six hundred
_case("hand_leaf1", [], hand=("leaf1", {"degenerate": True, "signed_zeros": True}), rays=True)
# ... and rays that meet the one leaf's box, flat in x = 0, at tFar = EPSILON5 exactly, one place above and one below: the
# walk's `tFar > EPSILON5`; the box is as thin as its face, so every ray that meets it has tNear == tFar (`tNear <= tFar`)
_case("hand_leaf1_box_edges", [("edge",)], hand=("leaf1", {"degenerate": True, "signed_zeros": True}), rays="box_edges")
_case("hand_chain300", [], hand=("chain300", {"degenerate": True, "signed_zeros": True}), rays=True)
_case("hand_chain300_lit_schlick", [("orb",), ("shadows",), ("differs", "hand_chain300_lit_schlick_noshadow")],
      hand=("chain300", {"degenerate": True, "signed_zeros": True, "lights": True, "brdf": 0}), set={"shadow_rays": 1}, rays=True)
_case("hand_chain300_lit_schlick_noshadow", [], hand=("chain300", {"degenerate": True, "signed_zeros": True, "lights": True, "brdf": 0}))

EPSILON5 = np.float32(0.00001)
EDGE_DISTANCES = np.array([EPSILON5, np.nextafter(EPSILON5, np.float32(1)), np.nextafter(EPSILON5, np.float32(0)), 2e-5, 1e-3, 0.5], np.float32)


def box_edge_rays(bvh, n=RAYS, seed=5):
    """n rays along +x and -x onto node 1's box, which is flat in x = 0: origins at x = -+EDGE_DISTANCES[k % 6], y and z
    inside the box but on none of its planes.  ( 0 - -e ) * ( 1 / 1 ) = e with no rounding: tNear = tFar = e."""
    lo, hi = bvh[1, 0:3].astype(np.float64), bvh[1, 4:7].astype(np.float64)
    assert lo[0] == 0.0 and hi[0] == 0.0 and (hi[1:] > lo[1:]).all()
    rng = np.random.default_rng(seed)
    side = np.where(np.arange(n) // EDGE_DISTANCES.size % 2 == 0, 1.0, -1.0)
    rays = np.zeros((n, 6), np.float32)
    rays[:, 0] = -side * EDGE_DISTANCES[np.arange(n) % EDGE_DISTANCES.size]
    rays[:, 1:3] = lo[1:] + (hi[1:] - lo[1:]) * rng.uniform(0.05, 0.95, (n, 2))
    rays[:, 3] = side
    return rays


_pbr = None


def _host():
    global _pbr
    if _pbr is None:
        import pbr_loader
        _pbr = pbr_loader.load()
    return _pbr


def _golden(name):
    with np.load(os.path.join(HERE, name + ".npz")) as d:
        return {k: d[k] for k in d.files}


_inputs = {}


def case_inputs(name):
    """The inputs of a case shaped like a ref_* fixture — the seven wire arrays, config (CONFIG_FIELDS), sky_light, camera
    (80 bytes), px_dim, seeds — plus first and rays ((n, 6) float32, n = 0 without a batch).  Shared; nobody writes to them."""
    if name in _inputs:
        return _inputs[name]
    spec = CASES[name]
    if "hand" in spec:
        frames = spec.get("frames", 3)
        import hand_scenes
        pbr = _host()
        shape, options = spec["hand"]
        sc = hand_scenes.scene(pbr, shape, **options)
        data = {k: np.ascontiguousarray(sc.arrays[k]) for k in WIRE}
        config = {f: float(getattr(sc.cfg, f)) for f in CONFIG_FIELDS}
        data["sky_light"] = np.array(list(sc.cfg.sky_light), np.float32)
        data["camera"] = np.frombuffer(bytes(sc.cam), np.uint8).copy()
        data["px_dim"] = np.float32(sc.px)
        data["seeds"] = np.asarray(pbr.frame_seeds(0, frames), np.float32)
        rays = box_edge_rays(data["bvh"]) if spec.get("rays") == "box_edges" else hand_scenes.rays_of(sc)
    else:
        base = _golden(spec["base"])
        frames = spec.get("frames", len(base["seeds"]))      # three, but two in the fixtures of the 8 k-face models
        data = {k: base[k] for k in WIRE + ("sky_light", "camera", "px_dim")}
        config = dict(zip(CONFIG_FIELDS, (float(v) for v in base["config"])))
        step = np.float32(base["seeds"][0])                  # the fixtures' seeds are k * 0.0333f, k = 1 ...: one more of them
        data["seeds"] = np.array([np.float32(np.float32(k + 1) * step) if k >= len(base["seeds"]) else base["seeds"][k] for k in range(frames)], np.float32)
        rays = base["rays"][:RAYS]
        if "geometry" in spec:
            g = _golden(spec["geometry"])
            for k in WIRE:
                data[k] = g["materials_schlick"] if (k == "materials" and config["brdf"] == 0) else g[k]
            assert data["lights"].shape[0] == base["lights"].shape[0] and np.array_equal(g["sky_light"], base["sky_light"])
    config.update(spec.get("set", {}))
    data["config"] = np.array([config[f] for f in CONFIG_FIELDS], np.float64)
    if "focus" in spec:
        cam = data["camera"].copy()
        cam.view(np.int32)[16:18] = spec["focus"]
        data["camera"] = cam
    data["first"] = int(spec.get("first", 0))
    data["rays"] = np.ascontiguousarray(rays if spec.get("rays") else np.zeros((0, 6)), np.float32)
    _inputs[name] = data
    return data


def centre_rays(data):
    """The rays through the pixel centres, no jitter, no lens: (h * w, 6) float32 from float64 arithmetic on the camera's fields."""
    c = dict(zip(CONFIG_FIELDS, data["config"]))
    w, h = int(c["width"]), int(c["height"])
    f = data["camera"].view(np.float32).astype(np.float64)
    eye, cw, cu, cv = f[0:3], f[4:7], f[8:11], f[12:15]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    inner = (cu - cu * w) + cu * (2.0 * xs[..., None]) + cv - cv * h + cv * (2.0 * ys[..., None])
    d = cw + inner * (float(data["px_dim"]) * 0.5)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.concatenate([np.broadcast_to(eye, d.shape), d], axis=-1).reshape(-1, 6).astype(np.float32)


def light_rays(data):
    """One ray from the first light — the one every shadow ray goes to — towards the middle of every face: ((faces, 6) float32,
    the distances in float64)."""
    v = data["vertices"][:, :3].astype(np.float64)
    middle = v[data["facesV"][:, :3].astype(np.int64)].mean(axis=1)
    origin = data["lights"][0, :3].astype(np.float64)
    d = middle - origin
    dist = np.linalg.norm(d, axis=1)
    return np.concatenate([np.broadcast_to(origin, d.shape), d / dist[:, None]], axis=1).astype(np.float32), dist


def light_census(dist, ray_t, ray_face):
    """[faces the light does not see — something else is hit clearly nearer —, faces it sees] of light_rays' closest hits."""
    seen = ray_face == np.arange(dist.size)
    return np.array([(~seen & (ray_t < 0.99 * dist)).sum(), seen.sum()], np.int64)


def values_of(data):
    """The compile-time placeholder texts of a case's inputs (oracle/refkernel.config_of)."""
    from oracle import refkernel
    c = dict(zip(CONFIG_FIELDS, data["config"]))
    ints = {f: int(c[f]) for f in ("width", "height", "brdf", "shadow_rays", "max_depth", "max_added_depth", "samples")}
    return refkernel.config_of(anti_aliasing=np.float32(c["anti_aliasing"]), phong_tessellation=np.float32(c["phong_tessellation"]),
                               sky_light=data["sky_light"], num_nodes=data["bvh"].shape[0], num_lights=data["lights"].shape[0], **ints)


def reference_outputs(name, scratch):
    """What the compiled reference kernel makes of a case: the arrays a fixture stores."""
    from oracle import refkernel
    data = case_inputs(name)
    values = values_of(data)
    out = refkernel.run(values, data, data["seeds"], data["first"], float(data["px_dim"]), data["camera"].tobytes(), data["rays"], scratch)
    if data["rays"].shape[0] == 0:
        out = {k: v for k, v in out.items() if not k.startswith("ray_")}
    if data["lights"].shape[0]:
        seen = refkernel.run(values, data, data["seeds"][:0], 0, float(data["px_dim"]), data["camera"].tobytes(), centre_rays(data), scratch)
        out["orb_pixels"] = np.int64((seen["ray_face"] < 0).sum())
        rays, dist = light_rays(data)
        lit = refkernel.run(values, data, data["seeds"][:0], 0, float(data["px_dim"]), data["camera"].tobytes(), rays, scratch)
        out["light_census"] = light_census(dist, lit["ray_t"], lit["ray_face"])
    keys = sorted(values)
    out["values_keys"], out["values_values"] = np.array(keys, dtype=str), np.array([values[k] for k in keys], dtype=str)
    return out


def recorded(name):
    return _golden("refkernel_" + name)


# ---- the walks per ray: refkernel_walk_<case>.npz -------------------------------------------------------------------------
# The reference's traverse (with a starting t) and traverseShadows on chosen rays (tests/walk_rays.py), through the trailer's
# rk_ray / rk_shadow_ray.  Stored per case: c_rays (n, 6), c_t0, c_t, c_face, c_counts {node visits, face tests} of the
# closest-hit walk; s_rays (m, 6), s_tlight, s_t, s_face, s_tests of the shadow walk; values_keys / values_values.  The rays ARE
# stored: the recordings are what the device is held to with nothing restated in between, and tests/test_walk_rays_cpu.py
# asserts that they are the constructors' own.
# name: (scene, rays) — scene: ("hand", shape, options) | ("fixture", ref_* name) | ("lanes", lights) | ("chain",);
# rays: "random" — WALK_RANDOM of walk_rays.random_set's rays, both walks on the same — | "edges" — the scene's edge classes |
# "inside" — walk_rays.inside_all_rays
WALK_RANDOM = 1024
WALK_CASES = {
    "hand_leaf1": (("hand", "leaf1", {"degenerate": True, "signed_zeros": True}), "random"),         # 2 nodes
    "hand_chain300": (("hand", "chain300", {"degenerate": True, "signed_zeros": True}), "random"),   # 603 nodes
    "suzanne_shadow": (("fixture", "ref_suzanne_sa_shadow"), "random"),                              # its orb light
    "inside_wide7": (("hand", "wide7", {"degenerate": True, "signed_zeros": True, "loose": True}), "inside"),   # every ray starts inside every box
    "lanes": (("lanes", False), "edges"),
    "lanes_lit": (("lanes", True), "edges"),
    "chain": (("chain",), "edges"),
}
WALK_SIZE_CAP = 256 * 1024


def walk_scene(name):
    """The scene of a walk case as a refit_scenes.Scene (desc, cfg, arrays), shared."""
    key = ("walk_scene", name)
    if key not in _inputs:
        import hand_scenes
        import refit_scenes
        import walk_rays
        pbr = _host()
        where = WALK_CASES[name][0]
        if where[0] == "hand":
            sc = hand_scenes.scene(pbr, where[1], **where[2])
        elif where[0] == "fixture":
            sc = refit_scenes.load(pbr, where[1])
        elif where[0] == "lanes":
            sc = walk_rays.lanes_scene(pbr, where[1])
        else:
            sc = walk_rays.chain_scene(pbr)
        _inputs[key] = sc
    return _inputs[key]


def walk_rays_of(name):
    """{c_rays, c_t0, s_rays, s_tlight} of a walk case, from tests/walk_rays.py."""
    import walk_rays
    sc, (where, kind) = walk_scene(name), WALK_CASES[name]
    if kind == "random":
        rays, t_light = walk_rays.random_set(sc)
        rays, t_light = rays[:WALK_RANDOM], t_light[:WALK_RANDOM]
        return {"c_rays": rays, "c_t0": np.full(rays.shape[0], np.inf, np.float32), "s_rays": rays, "s_tlight": t_light}
    if kind == "inside":
        closest, shadow = walk_rays.inside_all_rays(sc, False), walk_rays.inside_all_rays(sc, True)
        return {"c_rays": closest.rays, "c_t0": closest.t0, "s_rays": shadow.rays, "s_tlight": shadow.t0}
    closest, shadow = (walk_rays.lanes_rays(False, where[1]), walk_rays.lanes_rays(True, where[1])) if where[0] == "lanes" else \
        (walk_rays.chain_rays(False), walk_rays.chain_rays(True))
    return {"c_rays": closest.rays, "c_t0": closest.t0, "s_rays": shadow.rays, "s_tlight": shadow.t0}


def walk_values_of(name):
    sc = walk_scene(name)
    data = {"config": np.array([float(getattr(sc.cfg, f)) for f in CONFIG_FIELDS], np.float64), "sky_light": np.array(list(sc.cfg.sky_light), np.float32),
            "bvh": sc.arrays["bvh"], "lights": sc.arrays["lights"]}
    return values_of(data)


def walk_reference_outputs(name, scratch):
    """What the compiled reference's traverse and traverseShadows make of a walk case's rays: the arrays a recording stores."""
    from oracle import refkernel
    sc, rays = walk_scene(name), walk_rays_of(name)
    values = walk_values_of(name)
    out = refkernel.run(values, sc.arrays, np.zeros(0, np.float32), 0, float(sc.px), bytes(sc.cam), rays["c_rays"], scratch,
                        t0=rays["c_t0"], shadow_rays=np.concatenate([rays["s_rays"], rays["s_tlight"][:, None]], axis=1))
    keys = sorted(values)
    return dict(rays, c_t=out["ray_t"], c_face=out["ray_face"], c_counts=out["ray_counts"], s_t=out["shadow_t"], s_face=out["shadow_face"],
                s_tests=out["shadow_tests"], values_keys=np.array(keys, dtype=str), values_values=np.array([values[k] for k in keys], dtype=str))


def recorded_walk(name):
    return _golden("refkernel_walk_" + name)


def focus_w(name, out):
    x, y = CASES[name]["focus"]
    return float(out["image"][y, x, 3])


def reach_failures(name, outputs):
    """The REACH entries of a case that do not hold on `outputs` (name -> arrays): [text]."""
    bad = []
    for entry in REACH[name]:
        mine = outputs(name)
        if entry[0] == "equals":
            want = _golden(entry[1])
            for k in ("image", "debug", "ray_face", "ray_counts", "ray_t"):
                n = mine[k].shape[0]
                if not np.array_equal(mine[k], want[k][:n], equal_nan=True):
                    bad.append("%s: %s differs from %s" % (name, k, entry[1]))
        elif entry[0] == "differs":
            if np.array_equal(mine["image"][..., :3], outputs(entry[1])["image"][..., :3], equal_nan=True):
                bad.append("%s: the image equals %s's" % (name, entry[1]))
        elif entry[0] == "edge":
            e = np.abs(case_inputs(name)["rays"][:, 0])
            tests = mine["ray_counts"][:, 1]
            if not ((tests[e <= EPSILON5] == 0).all() and (tests[e > EPSILON5] >= 1).all() and (mine["ray_counts"][:, 0] == 1).all()
                    and min((e == d).sum() for d in EDGE_DISTANCES) >= RAYS // 8):
                bad.append("%s: the face tests do not start one place above tFar = EPSILON5" % name)
        elif entry[0] == "shadows":
            if not (mine["light_census"] > 0).all():
                bad.append("%s: the light sees every face or none (%s)" % (name, mine["light_census"].tolist()))
        elif entry[0] == "orb":
            if not int(mine["orb_pixels"]) > 0:
                bad.append("%s: no pixel-centre ray ends on an orb light" % name)
        elif entry[0] == "focus":
            w = focus_w(name, mine)
            if np.isfinite(w) != (entry[1] == "hit") or np.isnan(w):
                bad.append("%s: the focus pixel's .w is %r, wanted a %s" % (name, w, entry[1]))
    return bad


if __name__ == "__main__":
    import time
    from oracle import refkernel

    if not refkernel.available():
        sys.exit("the reference's sources are not on this machine")
    # the walk recordings (python tests/golden/make_refkernel.py --walk writes these alone and leaves refkernel_<case>.npz as they are)
    refkernel.build_many([walk_values_of(n) for n in WALK_CASES])
    with tempfile.TemporaryDirectory() as scratch:
        for name in WALK_CASES:
            out = walk_reference_outputs(name, scratch)
            path = os.path.join(HERE, "refkernel_walk_%s.npz" % name)
            np.savez_compressed(path, **out)
            assert os.path.getsize(path) < WALK_SIZE_CAP, path
            print("%-36s %6d bytes  %d closest-hit rays, %d hits; %d shadow rays, %d blocked" % (
                "walk_" + name, os.path.getsize(path), out["c_t"].size, np.isfinite(out["c_t"]).sum(), out["s_t"].size, (out["s_t"] < out["s_tlight"]).sum()))
    if "--walk" in sys.argv:
        sys.exit(0)
    t0 = time.time()
    refkernel.build_many([values_of(case_inputs(n)) for n in CASES], force=True)
    t1 = time.time()
    outs = {}
    with tempfile.TemporaryDirectory() as scratch:
        for name in CASES:
            outs[name] = reference_outputs(name, scratch)
    t2 = time.time()
    for name in CASES:
        path = os.path.join(HERE, "refkernel_%s.npz" % name)
        np.savez_compressed(path, **outs[name])
        assert os.path.getsize(path) < SIZE_CAP, path
        fails = reach_failures(name, outs.__getitem__)
        o = outs[name]
        print("%-36s %6d bytes  nodes/tris per frame %s  orb pixels %s  light census %s  focus .w %s  %s" % (
            name, os.path.getsize(path), o["frame_counts"].tolist(), o.get("orb_pixels", "-"), o["light_census"].tolist() if "light_census" in o else "-",
            focus_w(name, o) if "focus" in CASES[name] else "-", "; ".join(fails) or "reached: " + ", ".join(" ".join(e) for e in REACH[name])))
    print("%d cases, %d binaries: build %.1f s, run %.1f s" % (len(CASES), len({tuple(sorted(values_of(case_inputs(n)).items())) for n in CASES}), t1 - t0, t2 - t1))
