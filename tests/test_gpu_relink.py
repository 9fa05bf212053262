"""pbr_refit_ordered_walk on the GPU: pbr_update_vertices while a ray-ordered traversal is configured re-links the configured
layout's records on the device.  The contract (include/pbr_hip.h) is on bytes: context A — upload, configure( t ), flag on,
update — holds in pbr_diag_read_walk exactly what context B — upload, configure( 0 ), update, configure( t ), the host's packWalk
on the refitted tree — holds, header, first references and hot slots included.  Renders then equal a fresh upload's and the
oracle's in that mode; sequences, refusals, a large scene, and the temporal denoise's motion path under an ordered walk."""
import numpy as np
import pytest

import refit_ref
import refit_scenes
from conftest import same_values, describe_mismatch
from test_gpu_refit import bits, moved_scene, rays_for, rendered, assert_same_render
from test_gpu_temporal import cornell, view, MOVE
from test_gpu_temporal_motion import tall_block, translated, step, check_motion_step, BLOCK_MOVE

pytestmark = pytest.mark.gpu

LAYOUTS = (1, 2, 3)
SCENES = ("ref_suzanne_sa", "sponza_small", "ref_pillars_sa")


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


def relinked(dev, sc, layout, vertices):
    """Context A: upload, configure( layout ), flag on, update."""
    dev.upload_scene(sc.desc)
    dev.configure(sc.config(traversal=layout))
    dev.refit_ordered_walk(True)
    dev.update_vertices(vertices)


def through_the_host(dev, sc, layout, vertices):
    """Context B: upload, configure( 0 ), update, configure( layout )."""
    dev.upload_scene(sc.desc)
    dev.configure(sc.config(traversal=0))
    dev.update_vertices(vertices)
    dev.configure(sc.config(traversal=layout))


def assert_same_walk(a, b, what):
    (got, first, hot), (want, want_first, want_hot) = a.read_walk(), b.read_walk()
    assert got.size == want.size and got.size > 64, what
    if not np.array_equal(got, want):
        g, w = got.view(np.uint32), want.view(np.uint32)
        bad = np.nonzero(g != w)[0]
        raise AssertionError("%s: %d of %d words differ, the first at word %d: %08x, the host-built stream has %08x" % (what, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]]))
    assert first == want_first and hot == want_hot, what
    assert got[:32].view(np.int32).tolist() == first, what


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", SCENES)
def test_relinked_bytes_equal_the_host_built_stream(pbr, device, other, name, layout):
    """Both amplitudes, each from a new upload on the same pair of contexts."""
    sc = refit_scenes.load(pbr, name)
    before = None
    for amplitude in refit_ref.AMPLITUDES:
        v, moved = moved_scene(sc, amplitude)
        relinked(device, sc, layout, v)
        through_the_host(other, sc, layout, v)
        assert_same_walk(device, other, (name, layout, amplitude))
        info = device.relink_info()
        assert info["relinked"] and info["launches"] >= 3 and info["levels"] >= 1 and info["table_bytes"] > 0
        assert 0.0 < info["ms"] <= device.last_kernel_ms()
        assert np.array_equal(bits(device.read_bvh()), bits(moved.arrays["bvh"]))      # treeStale: read_bvh works as before
        assert_same_walk(device, other, (name, layout, amplitude, "after read_bvh"))
        now = device.read_walk()[0]
        assert before is None or not np.array_equal(now, before), "the second amplitude changed nothing"
        before = now


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ("ref_suzanne_sa", "sponza_small"))
def test_renders_equal_a_fresh_upload_and_the_oracle(pbr, oracle, device, other, name, layout):
    """A against a fresh upload of S' + configure( t ) and against the oracle's walk in that mode: image, debug image, counters,
    4096 single rays."""
    sc = refit_scenes.load(pbr, name)
    v, moved = moved_scene(sc, "large", seed=4)
    ordered = sc.config(traversal=layout)
    device.upload_scene(sc.desc)
    device.configure(ordered)
    device.render(0, sc.seeds, sc.px, sc.cam)              # the tuner and the dealing orders see the old scene
    device.refit_ordered_walk(True)
    device.update_vertices(v)
    other.upload_scene(moved.desc)
    other.configure(ordered)
    got = rendered(device, sc)
    assert_same_render(got, rendered(other, sc), "traversal %d against a fresh upload" % layout)
    ref = oracle.Renderer(moved.desc, ordered, threads=8)
    want = ref.render(0, sc.seeds, sc.px, sc.cam)
    assert_same_render(got, (want, ref.debug, ref.counter_dict()), "traversal %d against the oracle" % layout)
    rays = rays_for(v)
    mine, fresh = device.diag_trace(rays), other.diag_trace(rays)
    for a, b in zip(mine, fresh):
        assert same_values(a, b)
    t, face, normal, counts = mine
    want_t, want_face, want_normal, want_counts = oracle.trace_rays(moved.desc, ordered, rays)
    hit = np.isfinite(want_t)
    assert hit.sum() > 500
    assert same_values(t, want_t) and np.array_equal(counts, want_counts) and np.array_equal(face[hit], want_face[hit])
    a, fa = device.denoise(sc.px, sc.cam, features=True)
    b, fb = other.denoise(sc.px, sc.cam, features=True)
    assert same_values(a, b) and same_values(fa, fb)


def test_native_arithmetic_a_tile_shard_and_depth_of_field(pbr, device, other):
    """Each once, layout 2, A against a fresh upload of S': arith = native, tile shard 2 of 3, pbr_render_dof with a focus point."""
    if pbr.hip.pbr_mode_built(2, 1) != 1:
        pytest.fail("this build has no native-arithmetic kernels of the eight-order walk")
    sc = refit_scenes.load(pbr, "ref_suzanne_sa")
    v, moved = moved_scene(sc, "large", seed=8)
    for what, fields in (("native", dict(arith=1)), ("shard", dict(tile_world=3, tile_rank=2)), ("dof", {})):
        cfg = sc.config(traversal=2, **fields)
        device.upload_scene(sc.desc)
        device.configure(cfg)
        device.refit_ordered_walk(True)
        device.update_vertices(v)
        assert device.relink_info()["relinked"]
        other.upload_scene(moved.desc)
        other.configure(cfg)
        if what == "dof":
            cam = pbr.Camera.from_buffer_copy(sc.cam)
            cam.focusPoint[0], cam.focusPoint[1] = sc.cfg.width // 2, sc.cfg.height // 2
            for dev in (device, other):
                dev.reset_accum()
                dev.render_dof(0, pbr.frame_seeds(0, 3), sc.px, cam)
            assert same_values(device.read_output(), other.read_output()), describe_mismatch(device.read_output(), other.read_output())
        else:
            assert_same_render(rendered(device, sc), rendered(other, sc), what)


@pytest.mark.parametrize("layout", (1, 3))
def test_sequences_of_updates(pbr, device, other, layout):
    """V' then V'' == V'' alone; back to V == the host sequence with V (B, not the upload's bytes: tight boxes differ from the
    builder's); switching the layout after a re-linked update == a fresh upload."""
    sc = refit_scenes.load(pbr, "ref_suzanne_sa")
    a = sc.arrays
    v1, _ = moved_scene(sc, "large", seed=1)
    v2, moved2 = moved_scene(sc, "small", seed=2)
    relinked(device, sc, layout, v1)
    device.update_vertices(v2)
    relinked(other, sc, layout, v2)
    assert_same_walk(device, other, "V' V'' against V''")
    through_the_host(other, sc, layout, v2)
    assert_same_walk(device, other, "V' V'' against the host sequence")
    device.update_vertices(a["vertices"])
    through_the_host(other, sc, layout, a["vertices"])
    assert_same_walk(device, other, "back to V")
    # another layout: the existing host path, from the refreshed tree
    device.update_vertices(v2)
    switched = 2 if layout != 2 else 3
    device.configure(sc.config(traversal=switched))
    assert device.relink_info()["table_bytes"] == 0        # the tables went with the old layout's records
    through_the_host(other, sc, switched, v2)
    assert_same_walk(device, other, "switched to layout %d" % switched)
    other.upload_scene(moved2.desc)                         # a fresh upload ranks its hot nodes anew: the same renders, other bytes
    other.configure(sc.config(traversal=switched))
    assert_same_render(rendered(device, sc), rendered(other, sc), "switched to layout %d" % switched)
    device.update_vertices(v1)                              # and the new layout re-links with tables of its own
    through_the_host(other, sc, switched, v1)
    assert_same_walk(device, other, "layout %d re-linked" % switched)


def test_refusals_and_the_flag(pbr, device, other):
    """The flag is 0 after pbr_create, needs no scene, survives configure and upload; off, the update is refused as before; a
    refused update under the flag leaves the bytes and the renders as they were; relink_info tells when a re-link ran."""
    sc = refit_scenes.load(pbr, "ref_suzanne_sa")
    v = sc.arrays["vertices"]
    moved, _ = moved_scene(sc, "small")
    device.refit_ordered_walk(True)                         # no scene, not configured
    with pytest.raises(pbr.PbrError, match="-3: .*before pbr_upload_scene"):
        device.update_vertices(v)
    with pytest.raises(pbr.PbrError, match="-3: .*no ray-ordered stream"):
        device.read_walk()
    device.upload_scene(sc.desc)
    device.configure(sc.config(traversal=2))
    assert not device.relink_info()["relinked"] and device.relink_info()["table_bytes"] == 0
    before, walk = rendered(device, sc), device.read_walk()

    def unchanged(what):
        now = device.read_walk()
        assert np.array_equal(now[0], walk[0]) and now[1:] == walk[1:], what
        assert_same_render(rendered(device, sc), before, what)
        assert device.refit_info()["updates"] == 0

    assert pbr.hip.pbr_update_vertices(device._ctx, None, v.shape[0]) == -1
    unchanged("null vertices")
    with pytest.raises(pbr.PbrError, match="-1: .*%d vertices" % (v.shape[0] - 1)):
        device.update_vertices(v[:-1])
    unchanged("another count")
    w = moved.copy()
    w[v.shape[0] // 2, 2] = np.nan
    with pytest.raises(pbr.PbrError, match="-1: .*vertex %d is not finite" % (v.shape[0] // 2)):
        device.update_vertices(w)
    unchanged("a coordinate that is not finite")
    device.refit_ordered_walk(False)
    with pytest.raises(pbr.PbrError, match="-3: .*ray-ordered traversal"):
        device.update_vertices(moved)
    unchanged("flag off")
    # the flag survived the upload and the configure above; Phong tessellation stays refused under it
    device.refit_ordered_walk(True)
    device.configure(sc.config(traversal=2, phong_tessellation=0.6))
    with pytest.raises(pbr.PbrError, match="-3: .*Phong tessellation"):
        device.update_vertices(moved)
    device.configure(sc.config(traversal=2))
    device.upload_scene(sc.desc)
    device.update_vertices(moved)
    assert device.relink_info()["relinked"] and device.refit_info()["updates"] == 1
    through_the_host(other, sc, 2, moved)
    assert_same_walk(device, other, "after the refusals")
    # traversal 0 with the flag on: exactly the plain update, and it says so
    device.configure(sc.config(traversal=0))
    device.update_vertices(v)
    info = device.relink_info()
    assert not info["relinked"] and info["launches"] == 0 and info["ms"] == 0.0
    with pytest.raises(pbr.PbrError, match="-3: .*no ray-ordered stream"):
        device.read_walk()


def test_multi_driver_and_path_tracer_forward_the_flag(pbr, oracle, gpu_device):
    from importlib import import_module
    multi = import_module(pbr.__name__ + ".multi")
    sc = refit_scenes.load(pbr, "ref_pillars_sa")
    v, moved = moved_scene(sc, "small", seed=12)
    ordered = sc.config(traversal=2)
    want = oracle.Renderer(moved.desc, ordered, threads=8).render(0, sc.seeds, sc.px, sc.cam)
    m = multi.MultiDevice([gpu_device, gpu_device], multi.PEER_COPY)
    m.upload_scene(sc.desc)
    m.configure(ordered)
    with pytest.raises(pbr.PbrError):
        m.update_vertices(v)
    m.refit_ordered_walk(True)
    m.update_vertices(v)
    m.render(0, sc.seeds, sc.px, sc.cam)
    assert same_values(m.read_full(0), want)
    m.close()
    # the host driver forwards the flag to its context; its own configuration walks in the reference order
    pbr.cfg_reset()
    scene = pbr.HostScene.generate("cornell")
    pt = pbr.PathTracer(gpu_device, 32, 32)
    with pytest.raises(pbr.PbrError, match="before initOpenCLBuffers"):
        pt.refitOrderedWalk(True)
    pt.initOpenCLBuffers(scene)
    pt.refitOrderedWalk(True)
    arrays = scene.arrays()
    pt.updateVertices(refit_ref.deform(arrays["facesV"], arrays["vertices"], "small", seed=13))
    assert np.isfinite(pt.generateImages(1)[..., :3]).all()
    pt.refitOrderedWalk(False)
    pt.close()


def test_a_large_scene(pbr, device, other):
    """The generator and triangle count of test_gpu_refit's large scene: layout 2's bytes against the host sequence at the large
    amplitude and one 256 x 256 render against a fresh upload; layout 3 once, bytes only."""
    sc = refit_scenes.generated(pbr, "dragon", 4, 800000, 256, 256, **{"render.max_depth": 3})
    assert sc.arrays["facesV"].shape[0] >= 200000
    v, moved = moved_scene(sc, "large", seed=11)
    relinked(device, sc, 2, v)
    info = device.relink_info()
    assert info["relinked"] and info["levels"] > 10 and info["launches"] < info["levels"] + 2, info
    print("re-link of %d nodes, layout 2: %.3f ms of %.3f ms in %d launches, %d levels, %.1f MB of tables" %
          (sc.arrays["bvh"].shape[0], info["ms"], device.last_kernel_ms(), info["launches"], info["levels"], info["table_bytes"] / 1e6))
    through_the_host(other, sc, 2, v)
    assert_same_walk(device, other, "large scene, layout 2")
    other.upload_scene(moved.desc)
    other.configure(sc.config(traversal=2))
    device.pin_plan(4)
    other.pin_plan(4)
    assert_same_render(rendered(device, sc), rendered(other, sc), "large scene")
    relinked(device, sc, 3, v)
    through_the_host(other, sc, 3, v)
    assert_same_walk(device, other, "large scene, layout 3")


def test_temporal_motion_under_an_ordered_walk(pbr, device):
    """pbr_temporal_track_motion and the new flag under traversal 2: a static call, the tall block moves, a temporal call, it
    moves again with the camera, another — motion, history and integrated against tests/temporal_motion_ref.py, as
    test_gpu_temporal_motion checks the reference walk."""
    sc, cfg, px = cornell(pbr, device, traversal=2)
    temporal = pbr.TemporalParams()
    arrays = sc.arrays()
    faces, V0 = arrays["facesV"], arrays["vertices"]
    material, mask = tall_block(arrays)
    device.temporal_track_motion(True)
    device.refit_ordered_walk(True)
    prev = step(pbr, device, px, view(pbr, sc), 0, temporal)
    Hv = V0
    for k, move in enumerate([{}, MOVE]):
        V = translated(Hv, mask, BLOCK_MOVE)
        device.update_vertices(V)
        assert device.relink_info()["relinked"]
        s = step(pbr, device, px, view(pbr, sc, **move), 100 * (k + 1), temporal, motion=True)
        check_motion_step(s, prev, V, Hv, faces, temporal, "ordered walk, call %d" % (k + 2))
        hit = s.feat[1][..., 3] != 0
        on_block = hit & (faces[np.where(hit, s.face, 0), 3] == material)
        assert on_block.any() and (s.motion[..., 3][on_block] == 2).all() and (s.motion[..., 3][hit & ~on_block] == 1).all()
        prev, Hv = s, V
