"""The oracle's camera ray (orc_camera_ray: initRay, anti-aliasing jitter, depth-of-field lens) against the float64
restatement of the reference's formulas (tests/camera_ref.py): random pixels of a 1920 x 1080 image, and per image size,
anti-aliasing and aperture an edge set of corner and centre pixels, focus inputs and seeds whose first draw is 0 or next
to 1.  No GPU.  The GPU tests (test_gpu_camera_ref.py) reuse the generators and drivers below."""
import ctypes

import numpy as np
import pytest

import camera_ref as cr
import shading_ref as sr
from test_shading_ref_cpu import AMBIGUOUS_MAX, K_EXACT, MEDIAN_MAX, assert_ok, threshold_seeds

INF = np.float32(np.inf)
SIZES = [(8, 8), (64, 48), (1920, 1080)]          # 1920 x 1080: the largest size the suite configures
CONFIGS = [(w, h, aa, lense) for (w, h) in SIZES for aa in (0.0, 1.5) for lense in ((0.0, 8.0), (0.25, 2.0))]


class Setup:
    """One camera + configuration: the 18 values of camera_ref's tuple, and the pbr_camera / orc_camera wire struct."""

    def __init__(self, width, height, anti_aliasing, lense, focus=(-1, -1)):
        eye = np.array([0.13, 1.07, -3.21])
        look = np.array([-0.22, 0.31, 0.45]) - eye
        w = look / np.linalg.norm(look)
        u = np.cross(w, [0.0, 1.0, 0.0])
        u /= np.linalg.norm(u)
        v = np.cross(u, w)
        self.width, self.height, self.anti_aliasing = width, height, float(np.float32(anti_aliasing))
        self.px_dim = float(np.float32(2.0 * np.tan(np.radians(50.0) / 2) / height))
        self.cam = cr.camera_tuple(eye, w, u, v, lense, self.px_dim, anti_aliasing, width, height)
        wire = np.zeros(20, np.float32)
        wire[0:3], wire[4:7], wire[8:11], wire[12:15] = self.cam[cr.EYE], self.cam[cr.CW], self.cam[cr.CU], self.cam[cr.CV]
        wire[16:18] = np.array(focus, np.int32).view(np.float32)
        wire[18:20] = lense
        self.wire = wire

    def struct(self, cls):
        """The camera as an instance of the 80-byte ctypes structure cls."""
        assert ctypes.sizeof(cls) == self.wire.nbytes
        return cls.from_buffer_copy(self.wire.tobytes())


def items_of(px, py, seed, t_focus, t_object):
    it = np.zeros((len(px), 8), np.float32)
    it[:, 0], it[:, 1], it[:, 2], it[:, 3], it[:, 4] = px, py, seed, t_focus, t_object
    return it


def random_items(rng, setup, n=2048):
    focus = [np.float32(-1), np.float32(0), INF]
    pick = lambda: np.where(rng.integers(0, 4, n) == 0, rng.choice(focus, n), rng.uniform(0.5, 20, n).astype(np.float32))
    return items_of(rng.integers(0, setup.width, n), rng.integers(0, setup.height, n), rng.uniform(0, 300, n), pick(), pick())


def first_draw_seeds(randhash_exact):
    """Seeds whose FIRST draw is exactly 0 or as near 1 as the hash comes (sqrt( 1 - r ), sqrt( r ) of the jitter), and
    two plain ones."""
    seeds, what = threshold_seeds(randhash_exact)
    keep = [k for k, (j, target) in enumerate(what) if j == 0 and (target == 0.0 or target > 0.99)]
    assert len(keep) >= 4
    return np.concatenate([seeds[keep], np.float32([7.0, 123.25])])


def edge_items(setup, seeds):
    """The four corners and the four centre pixels x tFocus, tObject in {-1, 0, 1, INFINITY} x the seeds."""
    w, h = setup.width, setup.height
    pixels = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2 - 1, h // 2 - 1), (w // 2, h // 2 - 1), (w // 2 - 1, h // 2), (w // 2, h // 2)]
    focus = [np.float32(-1), np.float32(0), np.float32(1), INF]
    rows = [(px, py, s, tf, to) for (px, py) in pixels for tf in focus for to in focus for s in seeds]
    return items_of(*(np.array(c) for c in zip(*rows)))


class Cameras:
    """The implementation under test: fn( setup, items ) -> n x 8 and its hash; the oracle here, the device in
    test_gpu_camera_ref.py."""

    def __init__(self, fn, randhash, median_max=MEDIAN_MAX, ambiguous_max=AMBIGUOUS_MAX, flush=False):
        self.fn, self.randhash, self.median_max, self.ambiguous_max, self.flush = fn, randhash, median_max, ambiguous_max, flush

    def case(self, setup, items, K, random_batch=False):
        got = self.fn(setup, items)
        seq = sr.seed_sequence(items[:, 2])
        draws = self.randhash(seq[:, 1:].ravel()).reshape(-1, sr.DRAWS)
        res = cr.check(setup.cam, items, got, draws, seq, K, self.flush)
        res["got"] = got
        what = "camera ray %d x %d, anti-aliasing %g, lense %r" % (setup.width, setup.height, setup.anti_aliasing, setup.cam[cr.FOCAL:cr.APERTURE + 1])
        assert_ok(res, what, cr.inputs(items, draws), got, random_batch, self.median_max)
        # the seed after tells the draws taken: 2, or 4 with the lens (tFocus >= 0 and tObject > 0)
        lens = (items[:, 3] >= 0) & (items[:, 4] > 0)
        assert np.array_equal(got[:, 6], seq[np.arange(len(items)), np.where(lens, 4, 2)])
        assert (got[:, 7] == 0).all()
        return res


def summary(what, res):
    med = float(np.median(res["ratio"])) if res["ratio"].size else 0.0
    top = float(res["ratio"].max()) if res["ratio"].size else 0.0
    print("%s: median error / bound %.3g, largest %.3g, ambiguous share %.3g" % (what, med, top, float(res["ambiguous"].mean())))
    return top


def run_random(cameras, K, seed=0):
    rng = np.random.default_rng(900 + seed)
    tops = []
    for lense in ((0.25, 2.0), (0.0, 8.0)):
        setup = Setup(1920, 1080, 1.5, lense)
        res = cameras.case(setup, random_items(rng, setup), K, random_batch=True)
        tops.append(summary("camera ray, random batch, lense %r" % (lense,), res))
        assert res["ambiguous"].mean() <= cameras.ambiguous_max
    return max(tops)


def run_edges(cameras, K, randhash_exact):
    seeds = first_draw_seeds(randhash_exact)
    tops = []
    for w, h, aa, lense in CONFIGS:
        setup = Setup(w, h, aa, lense)
        res = cameras.case(setup, edge_items(setup, seeds), K)
        tops.append(summary("camera ray, edge set %d x %d aa %g lense %r" % (w, h, aa, lense), res))
    return max(tops)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle as the implementation under test
# ---------------------------------------------------------------------------------------------------------------------

def oracle_cameras(oracle):
    def fn(setup, items):
        return oracle.camera_ray(setup.width, setup.height, setup.anti_aliasing, setup.struct(oracle.OrcCamera), setup.px_dim, items)

    return Cameras(fn, lambda x: oracle.math("randhash", x))


def test_oracle_random_batches_match_float64(oracle):
    run_random(oracle_cameras(oracle), K_EXACT)


def test_oracle_edge_set_matches_float64(oracle):
    run_edges(oracle_cameras(oracle), K_EXACT, lambda x: oracle.math("randhash", x))


def test_first_draw_seeds_reach_their_targets(oracle):
    seeds = first_draw_seeds(lambda x: oracle.math("randhash", x))
    first = oracle.math("randhash", sr.seed_sequence(seeds)[:, 1])
    assert (first == 0).any() and (first > 1 - 2.0 ** -15).any()


def test_reference_sees_a_transcription_slip(oracle):
    """Not vacuous: the float64 result rounded to binary32 passes; one relative 1e-5 off — a hundredth of a pixel at
    1080 rows — fails on most samples; and so does a ray through the pixel's corner instead of its centre by 1 / 64 pixel."""
    setup = Setup(1920, 1080, 1.5, (0.25, 2.0))
    items = random_items(np.random.default_rng(4), setup, 512)
    seq = sr.seed_sequence(items[:, 2])
    draws = oracle.math("randhash", seq[:, 1:].ravel()).reshape(-1, sr.DRAWS)
    an = sr.Analysis(cr.camera_ray(items[:, 0], items[:, 1]), setup.cam, cr.inputs(items, draws), cr.CAM_KEYS)
    exact = np.zeros((512, 8), np.float32)
    exact[:, :6] = an.res["val"]
    exact[:, 6] = seq[np.arange(512), an.res["used"]]
    assert an.judge(exact, K_EXACT, seq).mean() > 0.999
    slipped = exact.copy()
    slipped[:, 3:6] *= np.float32(1 + 1e-5)
    assert an.judge(slipped, K_EXACT, seq).mean() < 0.5
    shifted = sr.Analysis(cr.camera_ray(items[:, 0] + 1.0 / 64, items[:, 1]), setup.cam, cr.inputs(items, draws), cr.CAM_KEYS).res["val"]
    moved = exact.copy()
    moved[:, :6] = shifted
    assert an.judge(moved, K_EXACT, seq).mean() < 0.5
