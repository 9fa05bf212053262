"""The device walks, the refit and the re-link over hand-made trees (tests/hand_scenes.py): a root with one child, containers
of 7 and 40 leaves, chains of height 301 and 1401, trees of 255 / 256 / 257 nodes around the refit's cut, a tree with a leaf
between two containers everywhere, trees of two nodes — with zeros of both signs, faces of three equal corners and boxes
that are all the scene's.  Everything is compared with references that take any nested tree: the oracle in the same
traversal, a float64 brute force over all faces, refit_ref / patch_refit_ref, and the host's packWalk through a second
context.  tests/test_hand_scenes_cpu.py holds what is assumed here about the inputs, the zero-outlier condition included.

32 x 24 images, two frames, depth 3, 2048 rays."""
import numpy as np
import pytest

import hand_scenes
import patch_refit_ref
import refit_ref
from conftest import same_values, describe_mismatch
from test_gpu_parity import PLANS
from test_gpu_refit import bits, rendered, assert_same_render
from test_gpu_relink import relinked, through_the_host, assert_same_walk
from hand_scenes import ALPHA
from test_scene_pack_cpu import STREAMS, RECORD_BYTES

pytestmark = pytest.mark.gpu

TRAVERSALS = (0, 1, 2, 3)
FAMILIES = ("refill-lean", "phased-mid", "phased-dual")          # one plan of each kernel family
LAYOUTS = (1, 2, 3)


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


@pytest.fixture()
def other(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def assert_same_rays(got, want, what):
    """pbr_diag_trace against the oracle's (or another context's): t and both counts as bits, face and normal on hits."""
    (t, face, normal, counts), (want_t, want_face, want_normal, want_counts) = got, want
    assert np.array_equal(bits(t), bits(want_t)), "%s t: %s" % (what, describe_mismatch(t, want_t))
    assert np.array_equal(counts, want_counts), "%s counts: %d rays differ" % (what, (counts != want_counts).any(axis=1).sum())
    hit = np.isfinite(want_t)
    assert np.array_equal(face[hit], want_face[hit]), what
    assert same_values(normal[hit], want_normal[hit]), what


def render_pinned(dev, sc, plan):
    dev.pin_plan(PLANS[plan])
    out = rendered(dev, sc)
    assert dev.last_plan()[0] == plan
    return out


def oracle_render(oracle, sc, cfg):
    ref = oracle.Renderer(sc.desc, cfg, threads=8)
    want = ref.render(0, sc.seeds, sc.px, sc.cam)
    return want, ref.debug, ref.counter_dict()


def cold_records(dev, nodes, layout):
    """The records behind the hot prefix, per stream, from pbr_diag_read_walk: the buffer is a 32-byte header, streams x
    ( nodes - 1 ) records and one record of padding; the hot prefix is counted in 32-byte slots."""
    data, _, hot_slots = dev.read_walk()
    size = RECORD_BYTES[layout]
    assert data.size == 32 + (STREAMS[layout] * (nodes - 1) + 1) * size
    hot = hot_slots * 32 // (size * STREAMS[layout])
    assert 0 < hot <= nodes - 1
    return nodes - 1 - hot


# ---- walks --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("boxes", ("tight", "loose"))
@pytest.mark.parametrize("shape", hand_scenes.SHAPES)
def test_single_rays_equal_the_oracle_and_the_brute_force(pbr, oracle, device, shape, boxes):
    """pbr_diag_trace in traversals 0 - 3 == orc_trace_rays in that mode — t and the node and face-test counts bit for bit,
    face and normal on hits — and the same rays lie within 1e-3 max( 1, t ) of Moeller-Trumbore over all faces in float64,
    none outside.  Under loose boxes every ray that hits anything visits every node: on chain1400 some 2800 one after the
    other, most of them cold in every ordered layout."""
    sc = dict(hand_scenes.walk_scenes(pbr, shape))[boxes]
    rays, best = hand_scenes.rays_of(sc), hand_scenes.brute_force_of(sc)
    device.upload_scene(sc.desc)
    for traversal in TRAVERSALS:
        cfg = sc.config(traversal=traversal)
        device.configure(cfg)
        got = device.diag_trace(rays)
        assert_same_rays(got, oracle.trace_rays(sc.desc, cfg, rays), "%s, %s boxes, traversal %d" % (shape, boxes, traversal))
        bad = hand_scenes.outliers(got[0], best)
        assert bad.size == 0, (shape, boxes, traversal, [(int(k), float(got[0][k]), float(best[k])) for k in bad[:4]])
        if traversal and shape == "chain1400":
            assert cold_records(device, sc.arrays["bvh"].shape[0], traversal) > 0
    assert np.isfinite(best).sum() >= hand_scenes.RAYS // 2
    assert device.guard_trips() == [0, 0, 0]


@pytest.mark.parametrize("boxes", ("tight", "loose"))
@pytest.mark.parametrize("shape", hand_scenes.SHAPES)
def test_renders_equal_the_oracle_in_every_kernel_family(pbr, oracle, device, shape, boxes):
    """Image, debug image and counters of refill-lean, phased-mid and phased-dual == oracle.Renderer's, traversals 0 - 3."""
    sc = dict(hand_scenes.walk_scenes(pbr, shape))[boxes]
    device.upload_scene(sc.desc)
    for traversal in TRAVERSALS:
        cfg = sc.config(traversal=traversal)
        device.configure(cfg)
        want = oracle_render(oracle, sc, cfg)
        assert want[2]["hits"] > 0
        for plan in FAMILIES:
            assert_same_render(render_pinned(device, sc, plan), want, "%s, %s boxes, traversal %d, %s" % (shape, boxes, traversal, plan))
    assert device.guard_trips() == [0, 0, 0]


@pytest.mark.parametrize("shape", hand_scenes.SHAPES)
def test_lit_renders_with_shadow_rays_equal_the_oracle(pbr, oracle, device, shape):
    """Both BRDFs with an orb light, a point light and shadow_rays = 1: the any-hit walk over the same trees."""
    for brdf in (0, 1):
        sc = hand_scenes.scene(pbr, shape, degenerate=True, signed_zeros=True, lights=True, brdf=brdf)
        device.upload_scene(sc.desc)
        for traversal, plan in zip((0, 2, 3), FAMILIES):
            cfg = sc.config(traversal=traversal, shadow_rays=1)
            device.configure(cfg)
            want = oracle_render(oracle, sc, cfg)
            assert_same_render(render_pinned(device, sc, plan), want, "%s, brdf %d, traversal %d, %s" % (shape, brdf, traversal, plan))
    assert device.guard_trips() == [0, 0, 0]


# ---- refit --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", hand_scenes.SHAPES)
def test_refit_equals_the_numpy_fold_and_a_fresh_upload(pbr, oracle, device, other, shape):
    """Upload with loose boxes, update_vertices( V' ): read_bvh() == refit_ref.refit, all eight words of every node as bits
    (zeros keep their sign); refit_info() shows the path the shape is there for; renders and single rays equal a fresh upload
    of S' in a second context and the oracle on S'; and back to V."""
    sc = hand_scenes.scene(pbr, shape, degenerate=True, signed_zeros=True, loose=True)
    a = sc.arrays
    nodes, height, _ = hand_scenes.EXPECT[shape]
    v, after = hand_scenes.moved(sc)
    device.upload_scene(sc.desc)
    device.configure(sc.cfg)
    info = device.refit_info()
    assert info["nested"] and info["subtree_cap"] == 256, info
    if nodes <= 256:
        assert info["top_levels"] == 0 and info["top_nodes"] == 0 and info["workgroups"] == 1 and info["subtrees"] == 1, info
    else:
        assert info["top_nodes"] >= 1 and info["top_levels"] >= 1, info
    if shape == "chain1400":
        assert info["top_levels"] > 1000, info
    if shape == "ternary10":
        assert info["subtrees"] > info["workgroups"] > 1, info
    device.update_vertices(v)
    got = device.read_bvh()
    assert np.array_equal(bits(got), bits(after.arrays["bvh"])), describe_mismatch(got, after.arrays["bvh"])
    other.upload_scene(after.desc)
    other.configure(sc.cfg)
    rays = hand_scenes.rays_at(a["facesV"], v, sc.flat, hand_scenes.RAYS, 5)
    mine = device.diag_trace(rays)
    assert_same_rays(mine, other.diag_trace(rays), shape + " against a fresh upload")
    assert_same_rays(mine, oracle.trace_rays(after.desc, sc.cfg, rays), shape + " against the oracle")
    assert np.isfinite(mine[0]).sum() >= hand_scenes.RAYS // 2
    want = oracle_render(oracle, after, sc.cfg)
    for plan in FAMILIES:
        image = render_pinned(device, sc, plan)
        assert_same_render(image, render_pinned(other, sc, plan), "%s, %s against a fresh upload" % (shape, plan))
        assert_same_render(image, want, "%s, %s against the oracle" % (shape, plan))
    device.update_vertices(a["vertices"])
    assert np.array_equal(bits(device.read_bvh()), bits(refit_ref.refit(a["bvh"], a["facesV"], a["vertices"])))
    assert device.refit_info()["updates"] == 2 and device.guard_trips() == [0, 0, 0]


# ---- re-link ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", hand_scenes.SHAPES)
def test_relink_equals_the_host_built_stream(pbr, oracle, device, other, shape, layout):
    """pbr_refit_ordered_walk on: after update_vertices( V' ) read_walk() is byte for byte what a second context builds through
    the host, and again after a second update that moves the keys back; the levels are the tree's height and a chain's share
    one launch; renders and single rays equal a fresh upload of S' and the oracle in that traversal."""
    sc = hand_scenes.scene(pbr, shape, degenerate=True, signed_zeros=True, loose=True)
    a = sc.arrays
    nodes, height, _ = hand_scenes.EXPECT[shape]
    v, after = hand_scenes.moved(sc)
    relinked(device, sc, layout, v)
    through_the_host(other, sc, layout, v)
    assert_same_walk(device, other, (shape, layout, "V'"))
    info = device.relink_info()
    assert info["relinked"] and info["levels"] == height and info["table_bytes"] > 0, info
    if shape.startswith("chain"):
        assert info["launches"] == 3, info                          # the sort, ALL levels, the records
    assert np.array_equal(bits(device.read_bvh()), bits(after.arrays["bvh"]))
    cold = cold_records(device, nodes, layout)
    if shape == "chain1400":
        assert cold > 0
    print("%s, layout %d: %d cold records per stream" % (shape, layout, cold))
    moved_walk = device.read_walk()[0]

    ordered = sc.config(traversal=layout)
    other.upload_scene(after.desc)
    other.configure(ordered)
    rays = hand_scenes.rays_at(a["facesV"], v, sc.flat, hand_scenes.RAYS, 5)
    mine = device.diag_trace(rays)
    assert_same_rays(mine, other.diag_trace(rays), "%s, layout %d against a fresh upload" % (shape, layout))
    assert_same_rays(mine, oracle.trace_rays(after.desc, ordered, rays), "%s, layout %d against the oracle" % (shape, layout))
    want = oracle_render(oracle, after, ordered)
    for plan in FAMILIES:
        image = render_pinned(device, sc, plan)
        assert_same_render(image, render_pinned(other, sc, plan), "%s, layout %d, %s against a fresh upload" % (shape, layout, plan))
        assert_same_render(image, want, "%s, layout %d, %s against the oracle" % (shape, layout, plan))

    device.update_vertices(a["vertices"])
    through_the_host(other, sc, layout, a["vertices"])
    assert_same_walk(device, other, (shape, layout, "back to V"))
    assert nodes == 2 or not np.array_equal(device.read_walk()[0], moved_walk), "the second update changed nothing"
    assert device.guard_trips() == [0, 0, 0]


# ---- Phong tessellation -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("traversal", (0, 2))
@pytest.mark.parametrize("shape", hand_scenes.PHONG_SHAPES)
def test_update_geometry_under_phong_tessellation(pbr, oracle, device, other, shape, traversal):
    """Distinct vertex normals, one face with equal normals, one without area, phong_tessellation 0.6: after
    update_geometry( V', N' ) read_bvh() == patch_refit_ref.refit and read_patches() == pack_patches as bits, and renders
    equal a fresh upload of S' and the oracle — in the reference walk, and in the eight-order walk behind the re-link."""
    sc, v, n, after = hand_scenes.phong_case(pbr, shape)
    a = sc.arrays
    thick = hand_scenes.with_arrays(sc, bvh=patch_refit_ref.refit(a["bvh"], a["facesV"], a["facesN"], a["vertices"], a["normals"], ALPHA))
    cfg = sc.config(traversal=traversal, phong_tessellation=ALPHA)
    device.refit_ordered_walk(traversal != 0)
    device.upload_scene(thick.desc)
    device.configure(cfg)
    device.update_geometry(v, n)
    got = device.read_bvh()
    assert np.array_equal(bits(got), bits(after.arrays["bvh"])), describe_mismatch(got, after.arrays["bvh"])
    assert np.array_equal(bits(device.read_patches()), bits(patch_refit_ref.pack_patches(a["facesV"], a["facesN"], v, n)))
    assert device.patch_refit_info()["alpha"] == np.float32(ALPHA)
    if traversal:
        assert device.relink_info()["relinked"] and device.relink_info()["levels"] == hand_scenes.EXPECT[shape][1]
        other.upload_scene(thick.desc)
        other.configure(sc.config(traversal=0, phong_tessellation=ALPHA))
        other.update_geometry(v, n)
        other.configure(cfg)
        assert_same_walk(device, other, (shape, "Phong tessellation"))
    other.upload_scene(after.desc)
    other.configure(cfg)
    image = rendered(device, sc)
    assert_same_render(image, rendered(other, sc), "%s, traversal %d against a fresh upload" % (shape, traversal))
    assert_same_render(image, oracle_render(oracle, after, cfg), "%s, traversal %d against the oracle" % (shape, traversal))
    rays = hand_scenes.rays_at(a["facesV"], v, sc.flat, hand_scenes.RAYS, 5)
    mine = device.diag_trace(rays)
    assert_same_rays(mine, other.diag_trace(rays), "%s, traversal %d against a fresh upload" % (shape, traversal))
    assert_same_rays(mine, oracle.trace_rays(after.desc, cfg, rays), "%s, traversal %d against the oracle" % (shape, traversal))
    assert image[2]["hits"] > 0 and np.isfinite(mine[0]).sum() > hand_scenes.RAYS // 4 and device.guard_trips() == [0, 0, 0]
