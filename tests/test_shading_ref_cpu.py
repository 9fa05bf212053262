"""The oracle's BRDF evaluation, new-ray sampling and surface step (orc_brdf_eval / orc_new_ray / orc_surface_step) against the float64 restatement of
the reference's formulas (tests/shading_ref.py): random batches like the GPU soak's, a fixed set of edge cases and
seeds whose draws land on the samplers' thresholds.  No GPU: this holds the oracle — and with it, through the bit-exact
parity tests, the HIP kernels' exact mode — to the reference's formulas, and holds the reference module itself to
something before any device is involved.  The GPU tests (test_gpu_shading_ref.py) reuse the drivers below."""
import ctypes

import numpy as np
import pytest

import shading_ref as sr

K_EXACT = 16            # error bounds per output: fixed before any GPU run (the exact arithmetic is a few ulp per operation)
MEDIAN_MAX = 2.0        # median of |got - ref| / ( 2^-24 |ref| + Delta ) over a random batch
AMBIGUOUS_MAX = 1e-4    # share of a random batch that may sit within an error bound of a branch threshold

_fp = ctypes.POINTER(ctypes.c_float)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------

def unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def random_directions(rng, n):
    """(normal, arriving out_dir, leaving in_dir) as the GPU soak draws them (test_gpu_math_exhaustive.py)."""
    normal = unit(rng.normal(size=(n, 3)))
    out_dir = unit(rng.normal(size=(n, 3)))
    out_dir -= 2 * np.maximum(0, (out_dir * normal).sum(1, keepdims=True)) * normal
    in_dir = unit(rng.normal(size=(n, 3)))
    in_dir += 2 * np.maximum(0, -(in_dir * normal).sum(1, keepdims=True)) * normal
    return normal.astype(np.float32), out_dir.astype(np.float32), in_dir.astype(np.float32)


def random_material(rng, brdf):
    """A material as the soak draws them: glass, mirrors and anisotropic lobes among them."""
    d = 1.0 if rng.integers(2) else float(rng.uniform(0, 1))
    ni = float(rng.uniform(1, 2))
    kd, ks = rng.uniform(0, 1, 3), rng.uniform(0, 1, 3)
    if brdf == 1:
        nu, nv = [0.0 if rng.integers(5) == 0 else float(10 ** rng.uniform(-1, 5)) for _ in range(2)]
        return np.asarray([d, ni, nu, nv, rng.uniform(0, 1), rng.uniform(0, 1), 0, 0, *kd, 0, *ks, 0], np.float32)
    return np.asarray([d, ni, rng.uniform(0.01, 1), rng.choice([0.0, 1.0, rng.uniform(0, 1)]), *kd, 0, *ks, 0], np.float32)


def material(brdf, d=1.0, ni=1.5, a=1.0, b=0.5, rs=0.5, rd=0.5):
    """BRDF 0: a = p (isotropy), b = rough; BRDF 1: a = nu, b = nv."""
    if brdf == 1:
        return np.asarray([d, ni, a, b, rs, rd, 0, 0, .5, .5, .5, 0, 1, 1, 1, 0], np.float32)
    return np.asarray([d, ni, a, b, .5, .5, .5, 0, 1, 1, 1, 0], np.float32)


def eval_items(normal, out_dir, in_dir):
    ev = np.zeros((normal.shape[0], 16), np.float32)
    ev[:, 0:3], ev[:, 3:6], ev[:, 6:9] = out_dir, in_dir, normal
    return ev


def ray_items(normal, dir_, origin, t, seed):
    nr = np.zeros((normal.shape[0], 12), np.float32)
    nr[:, 0:3], nr[:, 3:6], nr[:, 6:9], nr[:, 9], nr[:, 10] = origin, dir_, normal, t, seed
    return nr


def random_rays(rng, n):
    normal, out_dir, _ = random_directions(rng, n)
    nr = ray_items(normal, out_dir, rng.uniform(-1, 1, (n, 3)), rng.uniform(0.01, 5, n), rng.uniform(0, 300, n))
    nr[: n // 4, 6:9] *= -1                                  # back-facing normals too
    return nr


# --- the edge set ----------------------------------------------------------------------------------------------------

def edge_normals():
    axes = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    diag = np.float32(1 / np.sqrt(3))
    d3 = np.array([diag, diag, diag], np.float32)
    off = d3.copy()
    off[2] = np.nextafter(off[2], np.float32(1))
    return np.array(axes + [d3, -d3, off, -off, [0.6, 0.8, 0], [0, -0.28, 0.96]], np.float32)


def edge_directions():
    """(normal, out_dir, in_dir) triples: per edge normal a few arriving directions with in = reflect( out ) (h = n),
    grazing in and grazing out (perpendicular to n), generic pairs, and the same with the normal turned away."""
    rng = np.random.default_rng(5)
    rows = []
    for n in edge_normals().astype(np.float64):
        n = n / np.linalg.norm(n)
        t1 = np.cross(n, [0.3, -0.5, 0.81])
        t1 /= np.linalg.norm(t1)
        t2 = np.cross(n, t1)
        for k in range(4):
            out = unit(rng.normal(size=(1, 3)))[0]
            out = out - 2 * max(0, out @ n) * n
            rows.append((n, out, out - 2 * (out @ n) * n))                          # in = reflect( out ): dotHN == 1
            rows.append((n, out, t1 if k % 2 else t2))                              # grazing in: vIn = 0
            rows.append((n, (t2 if k % 2 else t1), unit(rng.normal(size=(1, 3)))[0] * np.array([1, 1, 1])))
            leave = unit(rng.normal(size=(1, 3)))[0]
            leave = leave + 2 * max(0, -(leave @ n)) * n
            rows.append((n, out, leave))
            rows.append((-n, out, leave))                                           # back-facing normal
    normal, out_dir, in_dir = (np.array([r[i] for r in rows], np.float32) for i in range(3))
    return normal, out_dir, in_dir


def edge_materials(brdf):
    if brdf == 1:
        lobes = [(0, 0), (1e5, 1e5), (1e4, 1), (1, 1e4), (100, 10)]
        return [material(1, d, ni, nu, nv) for (nu, nv) in lobes for d, ni in ((1, 1.5), (0, 2.4), (0.5, 1.0))]
    shapes = [(p, r) for p in (0.0, 0.5, 1.0) for r in (0.0, 0.5, 1.0)] + [(0.3, 0.04)]
    return [material(0, d, ni, p, r) for (p, r) in shapes for d, ni in ((1, 1.5), (0, 2.4), (0.5, 1.0))]


def critical_rays():
    """Glass at and within a few ulp of the critical angle, entering (Ni = 1 < NI_AIR) and leaving (Ni = 2.4), with
    d = 0: every sample refracts.  Returns [(material Ni, rays)]."""
    out = []
    for ni in (1.0, 2.4):
        m1, m2 = (sr.NI_AIR, float(np.float32(ni))) if ni < sr.NI_AIR else (float(np.float32(ni)), sr.NI_AIR)
        cos_c = np.sqrt(1 - (m2 / m1) ** 2)
        cos_i = cos_c + np.arange(-12, 13) * 2.0 ** -22                     # a few float32 ulp either side
        cos_i = np.clip(np.concatenate([cos_i, cos_c * np.array([0.5, 0.9, 0.99, 1.01, 1.1, 2.0])]), 0.0, 1.0)
        sin_i = np.sqrt(1 - cos_i ** 2)
        entering = ni < sr.NI_AIR
        d = np.stack([sin_i, np.zeros_like(sin_i), -cos_i if entering else cos_i], axis=1)
        n = len(d)
        normal = np.tile([0.0, 0.0, 1.0], (n, 1))
        rays = ray_items(normal.astype(np.float32), d.astype(np.float32), np.zeros((n, 3)), np.full(n, 1.0), 64.0 + np.arange(n) * 3.0)
        out.append((ni, rays))
    return out


_SEEDS = {}


def threshold_seeds(randhash):
    """Seeds s such that draw j (the ( j + 1 )-th value of the sequence, j = 0, 1, 2) lands within 1e-6 of 0.25, 0.5,
    0.75, exactly on 0, or as close below 1 as the hash comes: found in the exact hash.  Returns the seeds (float32) and,
    per seed, (j, target or draw reached).

    The largest float32 below 1 itself is out of reach: fract( sin( s ) * 43758.5453 ) comes within 2^-24 of 1 only for
    a product in [0.5, 1) rounded to 1 - 2^-24, and the float32 seeds near k pi are too coarse for that.  The search runs
    over the 4096 seeds around each k pi, k = 2 .. 3999, where small products live; the best draws it finds are
    1 - 1.5e-5 and a few more within 3.1e-5 of 1, where the Shirley-Ashikhmin sampler's tan( pi/2 * ( 1 - 4 ( 1 - a ) ) )
    is about 5e3 to 1e4.  Cached: the search is the same for every caller."""
    if "seeds" not in _SEEDS:
        x = (np.arange(1 << 22, dtype=np.uint32) + np.float32(64.0).view(np.uint32)).view(np.float32)
        h = randhash(x).astype(np.float64)
        picks = []
        for target in (0.25, 0.5, 0.75, 0.0):
            hit = np.flatnonzero(np.abs(h - target) <= 1e-6)
            assert hit.size >= 3, "no seed in the search range reaches %r" % target
            picks += [(float(x[i]), target) for i in hit[:3]]
        around = np.float32(np.arange(2, 4000) * np.pi).view(np.uint32)[:, None].astype(np.int64) + np.arange(-2048, 2048)
        x = around.astype(np.uint32).ravel().view(np.float32)
        h = randhash(x).astype(np.float64)
        picks += [(float(x[i]), float(h[i])) for i in np.argsort(h)[-3:]]
        seeds, what = [], []
        for xv, target in picks:
            for j in range(3):
                s = np.float32(xv) - np.float32(j + 1)
                assert sr.seed_sequence(np.array([s]))[0, j + 1] == np.float32(xv)
                seeds.append(s)
                what.append((j, target))
        _SEEDS["seeds"] = (np.array(seeds, np.float32), what)
    return _SEEDS["seeds"]


# ---------------------------------------------------------------------------------------------------------------------
# the driver: one stage, one material, one batch
# ---------------------------------------------------------------------------------------------------------------------

BRDF_MTL_KEYS = {0: (2, 3), 1: (2, 3, 5)}
RAY_MTL_KEYS = {0: (1, 2, 3), 1: (1, 2, 3)}


def brdf_inputs(ev):
    e = ev.astype(np.float64)
    return {"out": e[:, 0:3], "in": e[:, 3:6], "normal": e[:, 6:9]}


def ray_inputs(nr, draws):
    r = nr.astype(np.float64)
    return {"origin": r[:, 0:3], "dir": r[:, 3:6], "normal": r[:, 6:9], "t": r[:, 9], "draws": draws.astype(np.float64)}


def draws_for(randhash, seeds):
    seq = sr.seed_sequence(seeds)
    return randhash(seq[:, 1:].ravel()).reshape(-1, sr.DRAWS), seq


def check_brdf(brdf, mtl, ev, got, K, flush=False):
    m = sr.f32(mtl)
    return sr.check(sr.brdf_eval(brdf), m, brdf_inputs(ev), got, K, BRDF_MTL_KEYS[brdf], flush=flush)


SURFACE_MTL_KEYS = {0: (1, 2, 3, 4, 5, 6, 8, 9, 10), 1: (1, 2, 3, 4, 5, 8, 9, 10, 12, 13, 14)}
SURFACE_JUDGE_COLS = [0, 1, 2, 5, 6, 7, 8, 9, 10, 11, 3, 4]     # the hook's n x 12 as surface_step's val, then seed and addDepth


def surface_items(normal, dir_, light_dir, t, seed, color, lit, light_rgb):
    it = np.zeros((normal.shape[0], 24), np.float32)
    it[:, 3:6], it[:, 6:9], it[:, 9], it[:, 10], it[:, 11:14], it[:, 14] = dir_, normal, t, seed, color, lit
    it[:, 15:18], it[:, 18:21] = light_dir, light_rgb
    it[:, 0:3] = 0.25
    return it


def surface_inputs(it, draws):
    r = it.astype(np.float64)
    return {"dir": r[:, 3:6], "normal": r[:, 6:9], "color": r[:, 11:14], "lit": r[:, 14], "lightDir": r[:, 15:18],
            "lightRgb": r[:, 18:21], "draws": draws.astype(np.float64)}


def surface_seeds(it):
    """`seed += t` (pathtracing.cl:281), in binary32: where the step's draws start."""
    return (it[:, 10] + it[:, 9]).astype(np.float32)


def check_surface(brdf, mtl, it, got, draws, seq, K, flush=False):
    m = sr.f32(mtl)
    return sr.check(sr.surface_step(brdf), m, surface_inputs(it, draws), got[:, SURFACE_JUDGE_COLS], K, SURFACE_MTL_KEYS[brdf], seeds=seq, flush=flush)


def random_surface(rng, n, randhash):
    """Random surface steps, lit and unlit, a quarter with back-facing normals.  The draws are inputs, taken from the
    arithmetic under test: the hash has some 2^-9 of resolution (fract of a product near 4e4) and is exactly 0 once in a
    few hundred draws, where both samplers return the lobe's peak itself, h = n — the BRDFs' singular point.  The seeds are
    chosen so that none of a sample's draws is 0; what the samplers do with a draw of 0 is the threshold seeds' business."""
    m = 2 * n
    normal, out_dir, light_dir = random_directions(rng, m)
    normal[: m // 4] *= -1                                   # back-facing normals: the flip runs, the tangent frame is dropped
    it = surface_items(normal, out_dir, light_dir, rng.uniform(0.01, 5, m), rng.uniform(0, 300, m), rng.uniform(0, 1, (m, 3)),
                       rng.integers(0, 2, m), rng.uniform(0, 2, (m, 3)))
    draws, _ = draws_for(randhash, surface_seeds(it))
    keep = np.flatnonzero((draws > 0).all(axis=1))
    assert keep.size >= n
    return it[rng.permutation(keep)[:n]]


SOFT_LOBE = 10.0        # Shirley-Ashikhmin exponents up to this: see decided_material


def decided_material(rng, brdf):
    """A random material whose surface step has no singular point a sample can reach with probability above the cap:
    opaque (d = 1: no refracted or mirrored ray, whose evaluation has h = n or h = 0 / 0), and for Shirley-Ashikhmin both
    exponents at most SOFT_LOBE.  A lobe of exponent e puts ( e + 1 ) eps of its samples within 1 - dotHN <= eps of its
    peak, where the exponent of the evaluation is 0 / 0; with eps = K * 8 * 2^-24 — the error bound of a dot product of two
    normalised vectors — that is 8e-5 ( e + 1 ) in the exact and 2.4e-4 ( e + 1 ) in the native arithmetic, each against its
    cap of 1e-4 and 3.2e-3: e <= 10 keeps the native share inside, and the exact one inside for the batches of the suite."""
    while True:
        mtl = random_material(rng, brdf)
        mtl[0] = 1.0
        if brdf == 0 or max(mtl[2], mtl[3]) <= SOFT_LOBE:
            return mtl


def sampled_direction_bound(brdf, mtl, K, n):
    """An upper bound, from the material alone, of the share of a batch that may be ambiguous in the evaluation at the
    sampled direction, for the materials decided_material excludes: the refracting samples (a share 1 - d of the batch, three
    standard deviations added; every mirrored and every straight-through ray is among them) and, for Shirley-Ashikhmin,
    the samples within the error bound of the lobe's peak, ( max( nu, nv ) + 1 ) K 8 2^-24 (decided_material)."""
    d = float(mtl[0])
    bound = (1.0 - d) + 3.0 * np.sqrt(max(d * (1.0 - d), 0.0) / n)
    if brdf == 1:
        bound += (max(float(mtl[2]), float(mtl[3])) + 1.0) * K * 8.0 * sr.U
    return min(1.0, bound)


def edge_surface():
    """The BRDF edge directions (normals on the axes and next to +-(1,1,1), h = n, grazing, back-facing), and on top:
    the arriving ray along and against the normal and perpendicular to it, the light below the surface (the pdf cut),
    colours of 0 and above 1, lit and unlit.
    "Perpendicular" is 2^-12 either side of it, so that the flip runs either way and the tangent frame is reused and
    dropped: at exactly 0 the flip, the samplers' own tests of the same dot product and the BRDFs' vOut == 0 guards are all
    undecided at once, and `check` follows one undecided branch at a time."""
    normal, out_dir, in_dir = edge_directions()
    off = np.abs((normal.astype(np.float64) * out_dir).sum(1)) > 2.0 ** -20      # the exactly grazing triples: see below
    # ... and a normal exactly along +-(1,1,1): its tangent frame is normalize( 0 ), undefined in the reference (shading_ref);
    # the BRDF evaluation's own edge set keeps it, the normals an ulp off the diagonal stay here
    off &= ~((normal[:, 0] == normal[:, 1]) & (normal[:, 1] == normal[:, 2]))
    normal, out_dir, in_dir = normal[off], out_dir[off], in_dir[off]
    extra_n = edge_normals().astype(np.float64)
    extra_n = extra_n[~((extra_n[:, 0] == extra_n[:, 1]) & (extra_n[:, 1] == extra_n[:, 2]))]
    extra_n /= np.linalg.norm(extra_n, axis=1, keepdims=True)
    t1 = unit(np.cross(extra_n, [0.3, -0.5, 0.81]))
    leave = unit(extra_n + 0.5 * t1)
    tilt = 2.0 ** -12
    blocks = [(normal, out_dir, in_dir), (normal, out_dir, -in_dir),
              (extra_n, -extra_n, leave), (extra_n, extra_n, leave), (extra_n, unit(t1 - tilt * extra_n), leave),
              (extra_n, unit(t1 + tilt * extra_n), leave), (extra_n, -extra_n, -leave)]
    normal, out_dir, light = (np.concatenate([b[i] for b in blocks]).astype(np.float32) for i in range(3))
    n = normal.shape[0]
    colours = np.array([(0, 0, 0), (1, 1, 1), (2.5, 0.5, 1.5), (0.3, 0.6, 0.9)], np.float32)
    k = np.arange(n)
    return surface_items(normal, out_dir, light, np.full(n, 2.0), 17.0 + k * 1.5, colours[k % 4], (k // 4) % 2 == 0,
                         np.array([(1, 1, 1), (3, 2, 0.5), (0, 0, 0)], np.float32)[k % 3])


def check_new_ray(brdf, mtl, nr, got, draws, seq, K, flush=False):
    m = sr.f32(mtl)
    return sr.check(sr.new_ray(brdf), m, ray_inputs(nr, draws), got, K, RAY_MTL_KEYS[brdf], seeds=seq, flush=flush)


def assert_ok(res, what, x, got, random_batch=False, median_max=MEDIAN_MAX):
    an = res["analysis"]
    ref_finite = np.isfinite(an.res["val"]) & np.isfinite(an.delta)
    lost = (ref_finite & ~np.isfinite(got[:, :ref_finite.shape[1]])).any(axis=1) & ~res["ambiguous"]
    assert not lost.any(), "%s: NaN or Inf where the float64 reference is finite and bounded\n%s" % (
        what, sr.describe(dict(res, ok=~lost), x, got, what))
    assert res["ok"].all(), sr.describe(res, x, got, what)
    if random_batch:
        med = np.median(res["ratio"]) if res["ratio"].size else 0.0
        assert med <= median_max, "%s: median error %.3g bounds" % (what, med)


class Stages:
    """The stage implementation under test: the oracle here, the device in test_gpu_shading_ref.py."""

    def __init__(self, brdf_fn, ray_fn, randhash, median_max=MEDIAN_MAX, ambiguous_max=AMBIGUOUS_MAX, flush=False, surface_fn=None,
                 prepare=None):
        """flush: the arithmetic under test flushes subnormal results to 0.  prepare( brdf, mtl ): whatever randhash needs
        done before it is asked ahead of a stage call (the device: its configuration)."""
        self.brdf, self.ray, self.randhash, self.surface = brdf_fn, ray_fn, randhash, surface_fn
        self.prepare = prepare or (lambda brdf, mtl: None)
        self.median_max, self.ambiguous_max, self.flush = median_max, ambiguous_max, flush

    def brdf_case(self, brdf, mtl, ev, K, random_batch=False):
        got = self.brdf(brdf, mtl, ev)
        res = check_brdf(brdf, mtl, ev, got, K, self.flush)
        assert_ok(res, "brdf %d %r" % (brdf, mtl[:6].tolist()), brdf_inputs(ev), got, random_batch, self.median_max)
        return res

    def ray_case(self, brdf, mtl, nr, K, random_batch=False):
        got = self.ray(brdf, mtl, nr)
        draws, seq = draws_for(self.randhash, nr[:, 10])
        res = check_new_ray(brdf, mtl, nr, got, draws, seq, K, self.flush)
        assert_ok(res, "new ray %d %r" % (brdf, mtl[:6].tolist()), ray_inputs(nr, draws), got, random_batch, self.median_max)
        return res

    def surface_case(self, brdf, mtl, it, K, random_batch=False):
        got = self.surface(brdf, mtl, it)
        draws, seq = draws_for(self.randhash, surface_seeds(it))
        res = check_surface(brdf, mtl, it, got, draws, seq, K, self.flush)
        res["got"] = got
        assert_ok(res, "surface step %d %r" % (brdf, mtl[:6].tolist()), surface_inputs(it, draws), got[:, SURFACE_JUDGE_COLS], random_batch, self.median_max)
        return res


def input_ambiguous(res, K):
    """The samples with an ambiguous decision other than those inside the BRDF evaluation at the SAMPLED direction (the
    "N." decisions of shading_ref.surface_step)."""
    amb = np.zeros(res["analysis"].n, bool)
    for key, a in res["analysis"].ambiguous(K).items():
        if not key.startswith("N."):
            amb |= a
    return amb


def run_random_surface(stages, brdf, K, materials=6, n=2048, seed=0):
    """Surface steps over random materials and directions, lit and unlit.  Returns (median, largest) error / bound.

    Half the batches use decided_material: there EVERY decision of the step is held to the ambiguity cap, and the median is
    over whole batches.  The other half use random_material as it is — glass, sharp lobes —, where the evaluation at the
    SAMPLED direction reaches the BRDFs' singular set whatever the inputs: a mirrored ray (total reflection, reflectance >=
    draw) has h = n exactly, where the Schlick model's cross( cross( h, n ), n ) is the zero vector and its anisotropy term
    noise in the reference itself, and a sharp Shirley-Ashikhmin lobe samples its own peak, where the exponent is 0 / 0.
    There the decisions the inputs control (the samplers', the flip, the light's evaluation and its pdf cut) are held to the
    cap, the ambiguous share at the sampled direction to sampled_direction_bound — fixed by the material before the run —,
    and for the Schlick model every such sample must be one that refracted."""
    rng = np.random.default_rng(57 + brdf + 100 * seed)
    meds, top, ambiguous, total = [], 0.0, 0, 0
    for k in range(materials):
        decided = k < (materials + 1) // 2
        mtl = decided_material(rng, brdf) if decided else random_material(rng, brdf)
        stages.prepare(brdf, mtl)
        res = stages.surface_case(brdf, mtl, random_surface(rng, n, stages.randhash), K, random_batch=True)
        meds.append(float(np.median(res["ratio"])))
        top = max(top, float(res["ratio"].max()))
        by_input = input_ambiguous(res, K)
        sampled = res["ambiguous"] & ~by_input
        ambiguous, total = ambiguous + int((res["ambiguous"] if decided else by_input).sum()), total + n
        if not decided:
            bound = sampled_direction_bound(brdf, mtl, K, n)
            print("surface step, brdf %d %r: ambiguous share at the sampled direction %.3g, bound %.3g" % (brdf, mtl[:4].tolist(), sampled.mean(), bound))
            assert sampled.mean() <= bound + stages.ambiguous_max
            if brdf == 0:
                assert (sampled & ~res["analysis"].res["add"]).mean() <= stages.ambiguous_max
    share = ambiguous / float(total)
    print("surface step, brdf %d: median error / bound per material %s, largest %.3g, ambiguous share %.3g" % (
        brdf, [round(m, 3) for m in meds], top, share))
    assert share <= stages.ambiguous_max, "surface step %d: %d samples of %d ambiguous" % (brdf, ambiguous, total)
    return max(meds), top


def surface_edge_materials(brdf):
    """Every lobe shape of edge_materials at one of d = 1, 0, 0.5 in turn, and all three d for the first and the last."""
    m = edge_materials(brdf)
    return m[::3] + m[1::6] + m[2::6] + m[:3] + m[-3:]


def run_edges_surface(stages, brdf, K):
    it = edge_surface()
    top, meds, ambiguous, total = 0.0, [], 0, 0
    materials = surface_edge_materials(brdf)
    assert {float(m[0]) for m in materials} == {0.0, 0.5, 1.0}
    for mtl in materials:
        res = stages.surface_case(brdf, mtl, it, K)
        top = max(top, float(res["ratio"].max()) if res["ratio"].size else 0.0)
        meds.append(float(np.median(res["ratio"])) if res["ratio"].size else 0.0)
        ambiguous, total = ambiguous + int(res["ambiguous"].sum()), total + it.shape[0]
    print("surface step, brdf %d, edge set of %d per material: median error / bound %.3g (largest of %d materials), largest %.3g, ambiguous share %.3g" % (
        brdf, it.shape[0], max(meds), len(materials), top, ambiguous / float(total)))
    return top


def perpendicular_surface():
    """Arriving rays EXACTLY perpendicular to the normal, where binary32 is exact: normals on the axes, directions in the
    plane across (a product with an exact 0 is exact, so dot( normal, -dir ) is +-0 in any arithmetic), the light above and
    below, lit.  `dot( normal, -dir ) <= 0` flips the normal here and `< 0` would not: the one place that tells them apart,
    and the one place where the flip drops a tangent frame at equality."""
    rows = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            n = np.zeros(3)
            n[axis] = sign
            for a, b in ((1.0, 0.0), (0.0, -1.0), (0.6, 0.8), (-0.8, 0.6), (0.28, -0.96)):
                d = np.zeros(3)
                d[(axis + 1) % 3], d[(axis + 2) % 3] = a, b
                for up in (0.8, -0.8, 0.28):
                    light = 0.6 * np.roll(d, 1) * 0 + np.sqrt(1 - up * up) * np.cross(n, d) + up * n
                    rows.append((n, d, light))
    normal, dir_, light = (np.array([r[i] for r in rows], np.float32) for i in range(3))
    n = normal.shape[0]
    k = np.arange(n)
    colours = np.array([(1, 1, 1), (0.3, 0.6, 0.9), (2.5, 0.5, 1.5)], np.float32)
    return surface_items(normal, dir_, light, np.full(n, 2.0), 23.0 + k * 2.5, colours[k % 3], np.ones(n), np.array([(1, 1, 1), (3, 2, 0.5)], np.float32)[k % 2])


def perpendicular_materials(brdf):
    """Opaque ones: a translucent material hit at exactly grazing incidence reflects totally, the ray into itself, and the
    evaluation of that is 0 / 0 (shading_ref._half_vector)."""
    if brdf == 1:
        return [material(1, 1.0, 1.5, nu, nv) for nu, nv in ((0, 0), (3, 7), (100, 10))]
    return [material(0, 1.0, 1.5, p, r) for p, r in ((1.0, 0.2), (0.3, 0.04), (0.5, 1.0))]


def run_perpendicular_surface(stages, brdf, K):
    """Exactly perpendicular incidence.  In the exact arithmetic the verdict itself is asserted: the result must pass
    against the reference's own branch — flipped, the samplers' tests of the same +-0 taken as the reference takes them —
    with no alternative accepted; test_perpendicular_items_tell_the_flip_apart shows that the other branch would fail.
    In the native arithmetic either branch counts."""
    it = perpendicular_surface()
    for mtl in perpendicular_materials(brdf):
        res = stages.surface_case(brdf, mtl, it, K)
        an = res["analysis"]
        assert an.dec["U.flip"][0].all()
        if not stages.flush:
            _, seq = draws_for(stages.randhash, surface_seeds(it))
            # an item with some OTHER quantity within its bound of a threshold (a sampled ray on the horizon) keeps its
            # alternative; a quantity that is exactly 0 — the dot product in question, vOut — is no such case: binary32 has
            # the same 0; nor is a quantity that is NaN (the pdf of a light under the flipped normal: pow of a negative base)
            other = np.zeros(an.n, bool)
            for key, a in an.ambiguous(K).items():
                other |= a & ~(an.q[key][0] == 0.0) & ~np.isnan(an.q[key][0])
            assert other.mean() <= 0.1
            own = an.judge(res["got"][:, SURFACE_JUDGE_COLS], K, seq) | other
            assert own.all(), "surface step %d %r: exactly perpendicular items %s miss the reference's own branch" % (
                brdf, mtl[:6].tolist(), np.flatnonzero(~own).tolist())
        med = float(np.median(res["ratio"])) if res["ratio"].size else 0.0
        print("surface step, brdf %d %r, %d exactly perpendicular items: median error / bound %.3g, ambiguous share %.3g" % (
            brdf, mtl[:4].tolist(), it.shape[0], med, float(res["ambiguous"].mean())))


def run_random(stages, brdf, K, materials=12, n=2048, seed=0):
    rng = np.random.default_rng(31 + brdf + 100 * seed)
    stats, ambiguous = [], 0
    for _ in range(materials):
        mtl = random_material(rng, brdf)
        normal, out_dir, in_dir = random_directions(rng, n)
        r1 = stages.brdf_case(brdf, mtl, eval_items(normal, out_dir, in_dir), K, random_batch=True)
        r2 = stages.ray_case(brdf, mtl, random_rays(rng, n), K, random_batch=True)
        stats.append((np.median(r1["ratio"]), np.median(r2["ratio"])))
        ambiguous += int(r1["ambiguous"].sum() + r2["ambiguous"].sum())
    share = ambiguous / (2.0 * materials * n)
    assert share <= stages.ambiguous_max, "brdf %d: %d samples of %d ambiguous" % (brdf, ambiguous, 2 * materials * n)
    return stats


def run_edges(stages, brdf, K):
    normal, out_dir, in_dir = edge_directions()
    ev = eval_items(normal, out_dir, in_dir)
    n = normal.shape[0]
    nr = ray_items(normal, out_dir, np.full((n, 3), 0.25), np.full(n, 2.0), 17.0 + np.arange(n) * 1.5)
    for mtl in edge_materials(brdf):
        stages.brdf_case(brdf, mtl, ev, K)
        stages.ray_case(brdf, mtl, nr, K)
    for ni, rays in critical_rays():
        stages.ray_case(brdf, material(brdf, 0.0, ni, 1.0 if brdf == 0 else 10.0, 0.5 if brdf == 0 else 10.0), rays, K)


def run_threshold_seeds(stages, brdf, K, randhash_exact):
    seeds, _ = threshold_seeds(randhash_exact)
    rng = np.random.default_rng(11)
    normal, out_dir, _ = random_directions(rng, seeds.size)
    nr = ray_items(normal, out_dir, np.zeros((seeds.size, 3)), np.ones(seeds.size), seeds)
    for mtl in ([material(brdf, d, 1.5, *((0.4, 0.3) if brdf == 0 else (1e3, 10.0))) for d in (1.0, 0.5)]
                + [material(brdf, 1.0, 1.5, *((1.0, 0.2) if brdf == 0 else (1e5, 1e5)))]):
        stages.ray_case(brdf, mtl, nr, K)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle as the stage under test
# ---------------------------------------------------------------------------------------------------------------------

def oracle_stages(oracle):
    def brdf_fn(brdf, mtl, ev):
        out = np.empty((ev.shape[0], 4), np.float32)
        oracle.lib().orc_brdf_eval(brdf, mtl.ctypes.data, ev.ctypes.data_as(_fp), ev.shape[0], out.ctypes.data_as(_fp))
        return out

    def ray_fn(brdf, mtl, nr):
        out = np.empty((nr.shape[0], 8), np.float32)
        oracle.lib().orc_new_ray(brdf, mtl.ctypes.data, nr.ctypes.data_as(_fp), nr.shape[0], out.ctypes.data_as(_fp))
        return out

    return Stages(brdf_fn, ray_fn, lambda x: oracle.math("randhash", x), surface_fn=oracle.surface_step)


@pytest.mark.parametrize("brdf", [0, 1])
def test_oracle_random_batches_match_float64(oracle, brdf):
    stats = run_random(oracle_stages(oracle), brdf, K_EXACT)
    print("brdf %d: median error / bound per material (eval, new ray): %s" % (brdf, [(round(a, 3), round(b, 3)) for a, b in stats]))


@pytest.mark.parametrize("brdf", [0, 1])
def test_oracle_edge_set_matches_float64(oracle, brdf):
    run_edges(oracle_stages(oracle), brdf, K_EXACT)


@pytest.mark.parametrize("brdf", [0, 1])
def test_oracle_threshold_draws_match_float64(oracle, brdf):
    run_threshold_seeds(oracle_stages(oracle), brdf, K_EXACT, lambda x: oracle.math("randhash", x))


@pytest.mark.parametrize("brdf", [0, 1])
def test_oracle_surface_step_random_batches_match_float64(oracle, brdf):
    run_random_surface(oracle_stages(oracle), brdf, K_EXACT)


@pytest.mark.parametrize("brdf", [0, 1])
def test_oracle_surface_step_edge_set_matches_float64(oracle, brdf):
    run_edges_surface(oracle_stages(oracle), brdf, K_EXACT)


@pytest.mark.parametrize("brdf", [0, 1])
def test_oracle_surface_step_exactly_perpendicular_matches_float64(oracle, brdf):
    run_perpendicular_surface(oracle_stages(oracle), brdf, K_EXACT)


@pytest.mark.parametrize("brdf", [0, 1])
def test_perpendicular_items_tell_the_flip_apart(oracle, brdf):
    """Not vacuous: on the exactly perpendicular items the reference with the normal NOT flipped (`< 0` for `<= 0`) gives
    results that the reference's own branch rejects, for most items of every material."""
    it = perpendicular_surface()
    draws, seq = draws_for(lambda x: oracle.math("randhash", x), surface_seeds(it))
    idx = np.arange(it.shape[0])
    for mtl in perpendicular_materials(brdf):
        an = sr.Analysis(sr.surface_step(brdf), sr.f32(mtl), surface_inputs(it, draws), SURFACE_MTL_KEYS[brdf])
        other = an.subset(idx, "U.flip")
        wrong = np.zeros((it.shape[0], 12), np.float32)
        wrong[:, :10] = other.res["val"]
        wrong[:, 10] = seq[idx, other.res["used"]]
        wrong[:, 11] = other.res["add"]
        assert an.judge(wrong, K_EXACT, seq).mean() < 0.5, mtl[:6].tolist()


def test_threshold_seeds_reach_their_targets(oracle):
    """The search finds what it is for: draws within 1e-6 of each quadrant boundary, exactly 0, and near 1."""
    seeds, what = threshold_seeds(lambda x: oracle.math("randhash", x))
    seq = sr.seed_sequence(seeds)
    draws = oracle.math("randhash", seq[:, 1:].ravel()).reshape(-1, sr.DRAWS)
    for k, (j, target) in enumerate(what):
        assert abs(float(draws[k, j]) - target) <= 1e-6
    assert max(t for _, t in what) > 1 - 2.0 ** -15            # tan( pi/2 * a' ) > 5e3 for the SA sampler


def test_reference_sees_a_transcription_slip():
    """The comparison is not vacuous: the float64 result rounded to float32 passes it, and the same result one relative
    1e-5 off (a few hundred ulp, a slip far smaller than any of a formula's) fails it on most samples."""
    rng = np.random.default_rng(2)
    normal, out_dir, in_dir = random_directions(rng, 512)
    ev = eval_items(normal, out_dir, in_dir)
    mtl = material(1, 1.0, 1.5, 200.0, 20.0)
    an = sr.Analysis(sr.brdf_eval(1), sr.f32(mtl), brdf_inputs(ev), BRDF_MTL_KEYS[1])
    exact = an.res["val"].astype(np.float32)
    assert an.judge(exact, K_EXACT).mean() > 0.999
    assert an.judge(exact * np.float32(1 + 1e-5), K_EXACT).mean() < 0.5


@pytest.mark.parametrize("brdf", [0, 1])
def test_surface_reference_sees_a_transcription_slip(oracle, brdf):
    """Not vacuous for the surface step either: the float64 result rounded to binary32 passes; the colours one relative
    1e-5 off fail on most samples that have any."""
    rng = np.random.default_rng(6)
    mtl = material(brdf, 1.0, 1.5, *((0.4, 0.3) if brdf == 0 else (200.0, 20.0)))
    it = random_surface(rng, 512, lambda x: oracle.math("randhash", x))
    draws, seq = draws_for(lambda x: oracle.math("randhash", x), surface_seeds(it))
    an = sr.Analysis(sr.surface_step(brdf), sr.f32(mtl), surface_inputs(it, draws), SURFACE_MTL_KEYS[brdf])
    exact = np.zeros((512, 12), np.float32)
    exact[:, :10] = an.res["val"]
    exact[:, 10] = seq[np.arange(512), an.res["used"]]
    exact[:, 11] = an.res["add"]
    robust = np.isfinite(an.delta).all(axis=1) & (np.abs(exact[:, 3:6]).max(axis=1) > 0)
    assert robust.mean() > 0.5
    assert an.judge(exact, K_EXACT, seq).mean() > 0.999
    slipped = exact.copy()
    slipped[:, 3:9] *= np.float32(1 + 1e-5)
    assert an.judge(slipped, K_EXACT, seq)[robust].mean() < 0.5
