"""pbr_diag_trace_walk — the walk the lock-step render kernels run, one chosen ray per thread — on rays built for the edges of
its compares (tests/walk_rays.py; tests/test_walk_rays_cpu.py proves every class on the inputs and holds the oracle to the
reference's own compiled traverse / traverseShadows on the same rays).

Exact arithmetic: t and both counts as bits, face, and the normal on closest hits equal the oracle's in traversals 0 - 3, at
every staging level and wave shape, for both walks, with and without orb lights, and under Phong tessellation; in traversal
0 the recordings of the reference are compared directly.  Staged == unstaged == pbr_diag_trace; nothing depends on which
rays share a wave or on park_eighths.

Native arithmetic has no oracle.  What holds there: staged == unstaged bit for bit on every set (the hand-scheduled node phase
is the C++ loop's arithmetic, instruction for instruction), the random rays' verdicts equal a float64 brute force over all
faces wherever that decides, and the closest hit lies within four times the oracle's own distance from float64.

Measured on an MI355X, closest-hit max |t - t64| / max( 1, t64 ) over the decided random rays (the bound is four times the
oracle's figure), the same in traversals 0 - 3, staged and unstaged:

    tree        rays   oracle     native     rays whose bits differ from the oracle's
    leaf1       1793   5.62e-08   5.62e-08    0
    wide7       1704   1.56e-06   1.56e-06   41
    wide40      1732   3.34e-06   3.34e-06   54
    chain300    1748   8.14e-07   8.14e-07   46
    cut257      1731   1.44e-06   1.31e-06   44
    ternary10   1708   1.03e-06   3.42e-06   49      (bound 4.11e-06)
    generated   1772   1.57e-06   1.57e-06   15

On most trees the two agree to the digits printed: the largest distances are flatTriAndRayIntersect's moved origin
(tNear - 0.001 and back), which both arithmetics share, not a reciprocal; ternary10 shows the native one's own share.

On a build without the hand-scheduled node phase (PBR_GUARD) the staged path is the C++ loop over LDS: every test runs there
too and says in its output that the assembly was not reached.
"""
import os
import sys
import warnings

import numpy as np
import pytest

import hand_scenes
import walk_rays as wr
from conftest import same_values, describe_mismatch
from hand_scenes import ALPHA
from walk_rays import NATIVE_MARGIN, RANDOM_TREES, bits, random_scene

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_refkernel as mk              # noqa: E402

WALK_NAMES = sorted(mk.WALK_CASES)

pytestmark = pytest.mark.gpu

TRAVERSALS = (0, 1, 2, 3)
ABOVE = 1 << 20                       # more slots than any tree here has: clamped to the ranked prefix and the block's share of LDS
LEVELS = (0, 2, 3, 5, ABOVE)          # none; one record; counts that split a sibling pair (and, under traversal 3, a record: the even clamp)
PARTIAL = (1701, 1200)                # the generated scene: a few hundred records and more stay cold; odd: the even clamp again
LDS_SHARE = (160 * 1024 // 2 - 256) // 32     # a block's share of LDS at two blocks per CU, in slots: the entry's cap
NO_ASSEMBLY = "this build has no hand-scheduled node phase (PBR_GUARD): the staged walks ran the C++ loop over LDS — the assembly was NOT reached"
_reached = {}


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def assembly_reached(pbr, dev):
    """Whether this library's staged walk is the hand-scheduled node phase: the two-paths kernel exists only where it does
    (plan 6 renders with pathTracingDual there, with the six-waves state machine in a build without the assembly)."""
    if "asm" not in _reached:
        sc = hand_scenes.scene(pbr, "wide7", degenerate=True, signed_zeros=True)
        dev.upload_scene(sc.desc)
        dev.configure(sc.config(traversal=0))
        dev.pin_plan(6)
        dev.render(0, sc.seeds[:1], sc.px, sc.cam)
        _reached["asm"] = "pathTracingDual" in dev.last_kernel()
        dev.pin_plan(-1)
    if not _reached["asm"]:          # said by every test that asks: in the warnings summary of a passing run, and on its output
        warnings.warn(NO_ASSEMBLY)
        print("NOTE: " + NO_ASSEMBLY)
    return _reached["asm"]


def walk(dev, s, anyhit, slots, n=None):
    rays, t0 = (s.rays, s.t0) if n is None else (s.rays[:n], s.t0[:n])
    return dev.diag_trace_walk(rays, t0, anyhit=anyhit, lds_slots=slots)


def oracle_walk(oracle, sc, cfg, s, anyhit):
    return (oracle.trace_shadow_rays if anyhit else oracle.trace_rays)(sc.desc, cfg, s.rays, s.t0)


def assert_same_walk(got, want, anyhit, what):
    (t, face, normal, counts), (want_t, want_face, want_normal, want_counts) = got, want
    assert np.array_equal(bits(t), bits(want_t)), "%s t: %s" % (what, describe_mismatch(t, want_t))
    assert np.array_equal(counts, want_counts), "%s counts: rays %s differ" % (what, np.nonzero((counts != want_counts).any(axis=1))[0][:8].tolist())
    assert np.array_equal(face, want_face), "%s face: rays %s differ" % (what, np.nonzero(face != want_face)[0][:8].tolist())
    if not anyhit:
        assert same_values(normal, want_normal), "%s normal: %s" % (what, describe_mismatch(normal, want_normal))


def assert_same_bits(got, want, what):
    for k, name in enumerate(("t", "face", "normal", "counts")):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s %s: rays %s differ" % (
            what, name, np.nonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(a.shape[0], -1).any(axis=1))[0][:8].tolist())


class Set:
    def __init__(self, rays, t0):
        self.rays, self.t0, self.n = rays, np.ascontiguousarray(np.broadcast_to(np.asarray(t0, np.float32), (rays.shape[0],))), rays.shape[0]


def edge_sets(pbr):
    """(name, scene, anyhit, rays) of the hand-made scenes."""
    for lights in (False, True):
        sc = wr.lanes_scene(pbr, lights)
        for anyhit in (False, True):
            yield "lanes%s %s" % (" lit" if lights else "", "any-hit" if anyhit else "closest"), sc, anyhit, wr.lanes_rays(anyhit, lights)
    sc = wr.chain_scene(pbr)
    for anyhit in (False, True):
        yield "chain %s" % ("any-hit" if anyhit else "closest"), sc, anyhit, wr.chain_rays(anyhit)
    sc = wr.inside_scene(pbr)                     # every ray starts inside every box: tNear < 0 at every node
    for anyhit in (False, True):
        yield "inside %s" % ("any-hit" if anyhit else "closest"), sc, anyhit, wr.inside_all_rays(sc, anyhit)


# ---- exact arithmetic ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_edge_rays_equal_the_oracle_at_every_staging_level(pbr, oracle, device, traversal):
    reached = assembly_reached(pbr, device)
    for name, sc, anyhit, s in edge_sets(pbr):
        device.upload_scene(sc.desc)
        cfg = sc.config(traversal=traversal)
        device.configure(cfg)
        want = oracle_walk(oracle, sc, cfg, s, anyhit)
        for slots in LEVELS:
            assert_same_walk(walk(device, s, anyhit, slots), want, anyhit, "%s, traversal %d, %d slots%s" % (name, traversal, slots, "" if reached else " (no assembly)"))
    assert device.guard_trips() == [0, 0, 0]


@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_the_staging_levels_stage_what_they_are_there_for(pbr, device, traversal):
    """pbr_diag_trace_walk clamps a request to the ranked prefix, the block's share of LDS and, for compact records, an even
    count; pbr_diag_trace_walk_slots tells what it made of one.  On the generated scene: 2, 3, 5 are staged as asked (even under
    traversal 3), PARTIAL as asked and leaves more than 300 records of the stream cold, ABOVE is the whole prefix or the share."""
    sc = random_scene(pbr, "generated")
    device.upload_scene(sc.desc)
    device.configure(sc.config(traversal=traversal))
    even = (lambda k: k & ~1) if traversal == 3 else (lambda k: k)
    size = device.scene_bytes()
    stream_slots = (size["walk_streams"] if traversal else size["nodes"]) // 32
    record_slots = 2 if traversal == 3 else 1
    hot = device.diag_trace_walk_slots(0)[1]
    assert device.diag_trace_walk_slots(0)[0] == 0 and 0 < hot <= stream_slots
    for ask in LEVELS[1:-1] + PARTIAL:
        got = device.diag_trace_walk_slots(ask)[0]
        assert got == even(ask) and (traversal != 3 or ask % 2 == 0 or got == ask - 1), (traversal, ask, got)
    for ask in PARTIAL:
        assert (stream_slots - device.diag_trace_walk_slots(ask)[0]) // record_slots > 300, (traversal, ask, stream_slots)
    assert device.diag_trace_walk_slots(ABOVE)[0] == even(min(hot, LDS_SHARE)) > max(PARTIAL)


@pytest.mark.parametrize("name", WALK_NAMES)
def test_traversal_0_equals_the_recorded_reference_walks(pbr, device, name):
    """The device against what the reference's own compiled traverse / traverseShadows recorded: nothing restated in between."""
    assembly_reached(pbr, device)
    sc, rec = mk.walk_scene(name), mk.recorded_walk(name)
    device.upload_scene(sc.desc)
    device.configure(sc.config(traversal=0))
    for slots in (0, 2, ABOVE):
        t, face, _, counts = device.diag_trace_walk(rec["c_rays"], rec["c_t0"], anyhit=False, lds_slots=slots)
        assert np.array_equal(bits(t), bits(rec["c_t"])) and np.array_equal(face, rec["c_face"]) and np.array_equal(counts, rec["c_counts"]), (name, slots)
        t, face, _, counts = device.diag_trace_walk(rec["s_rays"], rec["s_tlight"], anyhit=True, lds_slots=slots)
        assert np.array_equal(bits(t), bits(rec["s_t"])), (name, slots, describe_mismatch(t, rec["s_t"]))
        assert np.array_equal(face, rec["s_face"]) and np.array_equal(counts[:, 1], rec["s_tests"]) and (counts[:, 0] == 0).all(), (name, slots)


@pytest.mark.parametrize("tree", RANDOM_TREES)
def test_random_rays_equal_the_oracle_staged_unstaged_and_diag_trace(pbr, oracle, device, tree):
    """Both walks in traversals 0 - 3; on the generated scene a staged prefix that leaves records cold."""
    assembly_reached(pbr, device)
    sc = random_scene(pbr, tree)
    rays, t_light = wr.random_set(sc)
    device.upload_scene(sc.desc)
    for traversal in TRAVERSALS:
        cfg = sc.config(traversal=traversal)
        device.configure(cfg)
        closest, shadow = Set(rays, np.inf), Set(rays, t_light)
        want_c, want_s = oracle_walk(oracle, sc, cfg, closest, False), oracle_walk(oracle, sc, cfg, shadow, True)
        assert_same_walk(device.diag_trace(rays), want_c, False, "%s, traversal %d, pbr_diag_trace" % (tree, traversal))
        for slots in (0, 3, ABOVE) + (PARTIAL if tree == "generated" else ()):
            assert_same_walk(walk(device, closest, False, slots), want_c, False, "%s closest, traversal %d, %d slots" % (tree, traversal, slots))
            assert_same_walk(walk(device, shadow, True, slots), want_s, True, "%s any-hit, traversal %d, %d slots" % (tree, traversal, slots))
    assert device.guard_trips() == [0, 0, 0]


@pytest.mark.parametrize("shape", hand_scenes.PHONG_SHAPES)
def test_phong_tessellation_equals_the_oracle(pbr, oracle, device, shape):
    """The Phong shapes under the thick boxes of their alpha: curved faces as patches in both walks, the hit's own normal."""
    assembly_reached(pbr, device)
    sc = hand_scenes.phong_case(pbr, shape)[3]
    rays, t_light = wr.random_set(sc, n=1024)
    device.upload_scene(sc.desc)
    for traversal in TRAVERSALS:
        cfg = sc.config(traversal=traversal, phong_tessellation=ALPHA)
        device.configure(cfg)
        closest, shadow = Set(rays, np.inf), Set(rays, t_light)
        want_c, want_s = oracle_walk(oracle, sc, cfg, closest, False), oracle_walk(oracle, sc, cfg, shadow, True)
        # the patches are met (not claimed of leaf2: its two faces are the case's face with equal normals and its face without area)
        assert shape == "leaf2" or not np.array_equal(bits(want_c[0]), bits(oracle.trace_rays(sc.desc, sc.config(traversal=traversal), rays)[0]))
        for slots in (0, ABOVE):
            assert_same_walk(walk(device, closest, False, slots), want_c, False, "%s closest, traversal %d, %d slots" % (shape, traversal, slots))
            assert_same_walk(walk(device, shadow, True, slots), want_s, True, "%s any-hit, traversal %d, %d slots" % (shape, traversal, slots))
    assert device.guard_trips() == [0, 0, 0]


def shapes_of(s, rng):
    """The same rays in other launches: (what, indices into the set) — 1, 63, 64 and 65 rays; 64 copies of one ray; the
    set in another order, so that other rays share a wave."""
    for n in (1, 63, 64, 65):
        if n <= s.n:
            yield "%d rays" % n, np.arange(n)
    for k in rng.integers(0, s.n, 2):
        yield "64 copies of ray %d" % k, np.full(64, k)
    yield "shuffled", rng.permutation(s.n)
    yield "reversed", np.arange(s.n)[::-1]


@pytest.mark.parametrize("arith", (0, 1))
@pytest.mark.parametrize("traversal", (0, 2, 3))
def test_results_do_not_depend_on_the_wave_shape_or_the_park_share(pbr, device, traversal, arith):
    """Per ray the same bits whichever rays share its wave (n = 1 makes keep = 0; 64 copies park in the same visit; on the
    chain lane i leaves after i pairs, and one long walk sits among 63 that miss node 1) and whatever share of a wave parks
    before the leaf phase (park_eighths 0, the default, 8) — in both arithmetics."""
    assembly_reached(pbr, device)
    rng = np.random.default_rng(9)
    sets = list(edge_sets(pbr))
    tree = random_scene(pbr, "chain300")
    rays, t_light = wr.random_set(tree)
    sets += [("chain300 random closest", tree, False, Set(rays[:512], np.inf)), ("chain300 random any-hit", tree, True, Set(rays[:512], t_light[:512]))]
    for name, sc, anyhit, s in sets:
        device.upload_scene(sc.desc)
        device.configure(sc.config(traversal=traversal, arith=arith))
        device.set_knob("park_eighths", -1)
        base = walk(device, s, anyhit, ABOVE)
        for what, idx in shapes_of(s, rng):
            got = device.diag_trace_walk(s.rays[idx], s.t0[idx], anyhit=anyhit, lds_slots=ABOVE)
            assert_same_bits(got, tuple(a[idx] for a in base), "%s, traversal %d, arith %d, %s" % (name, traversal, arith, what))
        for share in (0, 8):
            device.set_knob("park_eighths", share)
            for slots in (0, ABOVE):
                assert_same_bits(walk(device, s, anyhit, slots), base, "%s, traversal %d, arith %d, park_eighths %d, %d slots" % (name, traversal, arith, share, slots))
        device.set_knob("park_eighths", -1)
    assert device.guard_trips() == [0, 0, 0]


# ---- native arithmetic ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("traversal", TRAVERSALS)
def test_native_staged_equals_unstaged_on_every_set(pbr, device, traversal):
    """Bit for bit, the edge sets included: the one claim that holds without an oracle."""
    reached = assembly_reached(pbr, device)
    sets = list(edge_sets(pbr))
    for tree in ("wide7", "chain300", "generated"):
        sc = random_scene(pbr, tree)
        rays, t_light = wr.random_set(sc)
        sets += [(tree + " random closest", sc, False, Set(rays, np.inf)), (tree + " random any-hit", sc, True, Set(rays, t_light))]
    for name, sc, anyhit, s in sets:
        device.upload_scene(sc.desc)
        device.configure(sc.config(traversal=traversal, arith=1))
        base = walk(device, s, anyhit, 0)
        for slots in LEVELS[1:] + (PARTIAL if name.startswith("generated") else ()):
            assert_same_bits(walk(device, s, anyhit, slots), base, "%s, traversal %d, native, %d slots%s" % (name, traversal, slots, "" if reached else " (no assembly)"))
    assert device.guard_trips() == [0, 0, 0]


@pytest.mark.parametrize("tree", RANDOM_TREES)
def test_native_random_rays_agree_with_float64_where_it_decides(pbr, device, tree):
    assembly_reached(pbr, device)
    sc = random_scene(pbr, tree)
    rays, t_light = wr.random_set(sc)
    decided, blocked, t64, edge = wr.shadow_truth64(sc, rays, t_light, NATIVE_MARGIN)
    assert decided.mean() >= 0.95
    device.upload_scene(sc.desc)
    for traversal in TRAVERSALS:
        device.configure(sc.config(traversal=traversal, arith=1))
        for slots in (0, ABOVE):
            t = device.diag_trace_walk(rays, t_light, anyhit=True, lds_slots=slots)[0]
            wrong = decided & ((t < t_light) != blocked)
            assert not wrong.any(), (tree, traversal, slots, np.nonzero(wrong)[0][:4].tolist())


def relative_distance(t, t64, on):
    t = np.asarray(t, np.float64)
    with np.errstate(invalid="ignore"):
        return float(np.max(np.where(on, np.abs(t - t64) / np.maximum(1.0, t64), 0.0)))


@pytest.mark.parametrize("tree", RANDOM_TREES)
def test_native_closest_hits_stay_near_float64(pbr, oracle, device, tree):
    """|t - t64| / max( 1, t64 ) over the rays whose closest hit float64 decides (a hit clear of every boundary, a runner-up not
    within the guard): printed, and asserted against four times the largest value the ORACLE shows on the same rays — native
    rcp and sqrt are a few ulp where the exact ones are half an ulp."""
    assembly_reached(pbr, device)
    sc = random_scene(pbr, tree)
    rays, _ = wr.random_set(sc)
    a = sc.arrays
    t64, face, gap, edge = hand_scenes.brute_force_faces(a["facesV"], a["vertices"], np.asarray(rays, np.float64))
    on = (face >= 0) & (edge >= NATIVE_MARGIN) & (gap > wr.wt.T_GUARD) & (t64 > wr.wt.T_GUARD)
    assert on.sum() >= rays.shape[0] // 2
    want = oracle.trace_rays(sc.desc, sc.config(traversal=0), rays)[0]
    bound = 4.0 * relative_distance(want, t64, on)
    device.upload_scene(sc.desc)
    for traversal in TRAVERSALS:
        device.configure(sc.config(traversal=traversal, arith=1))
        for slots in (0, ABOVE):
            t = device.diag_trace_walk(rays, np.inf, anyhit=False, lds_slots=slots)[0]
            worst = relative_distance(t, t64, on)
            print("%s, traversal %d, %d slots: native %.3g, oracle %.3g (bound %.3g) over %d rays, %d of them differ from the oracle's bits" % (
                tree, traversal, slots, worst, bound / 4.0, bound, on.sum(), (bits(t) != bits(want))[on].sum()))
            assert np.isfinite(t[on]).all() and worst <= bound, (tree, traversal, slots, worst, bound)
