"""pbr_update_vertices on the GPU: the refitted boxes equal the numpy restatement of the fold (tests/refit_ref.py) bit for bit,
and an updated context behaves exactly like a fresh upload of the moved scene S' — against the oracle on S', and context
against context, in every render call, both BRDFs, with lights and shadow rays, pinned plans and the tuner, the ordered walks
configured afterwards, native arithmetic, tile sharding and chunked launches; every refusal leaves the context as it was."""
import ctypes

import numpy as np
import pytest

import refit_ref
import refit_scenes
from conftest import same_values, describe_mismatch
from test_scene_pack_cpu import hand_tree, NOT_NESTED

pytestmark = pytest.mark.gpu

GEOMETRIES = ("ref_pillars_sa", "ref_spheres_schlick", "ref_suzanne_sa", "sponza_small", "hairball_small", "cornell_sa")
# BRDF 1 / 0, with lights + shadow rays (suzanne_*_shadow) and without
PARITY = ("ref_suzanne_sa_shadow", "ref_suzanne_schlick_shadow", "ref_pillars_sa", "ref_spheres_schlick", "sponza_small", "cornell_schlick")


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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def moved_scene(sc, amplitude, seed=3):
    a = sc.arrays
    v = refit_ref.deform(a["facesV"], a["vertices"], amplitude, seed)
    return v, sc.moved(v, refit_ref.refit(a["bvh"], a["facesV"], v))


def rays_for(vertices, n=4096, seed=17):
    rng = np.random.default_rng(seed)
    lo, hi = vertices[:, :3].min(0) - 0.2, vertices[:, :3].max(0) + 0.2
    rays = np.concatenate([rng.uniform(lo, hi, (n, 3)), rng.normal(size=(n, 3))], axis=1).astype(np.float32)
    rays[:, 3:] /= np.linalg.norm(rays[:, 3:], axis=1, keepdims=True)
    return rays


def rendered(dev, sc, seeds=None):
    """(image, debug image, counters) of a fresh accumulation of sc's frames."""
    dev.reset_accum()
    dev.render(0, sc.seeds if seeds is None else seeds, sc.px, sc.cam)
    return dev.read_output(), dev.read_debug(), dev.counters()


def assert_same_render(a, b, what=""):
    assert same_values(a[0], b[0]), what + " image: " + describe_mismatch(a[0], b[0])
    assert same_values(a[1], b[1]), what + " debug image: " + describe_mismatch(a[1], b[1])
    assert a[2] == b[2], what + " counters"


@pytest.mark.parametrize("amplitude", refit_ref.AMPLITUDES)
@pytest.mark.parametrize("name", GEOMETRIES)
def test_read_bvh_equals_the_numpy_fold(pbr, device, name, amplitude):
    """Before any update pbr_read_bvh returns the uploaded nodes; after one, refit_ref's — all eight words of every node."""
    sc = refit_scenes.load(pbr, name)
    device.upload_scene(sc.desc)
    assert np.array_equal(bits(device.read_bvh()), bits(sc.arrays["bvh"]))
    info = device.refit_info()
    assert info["nested"] and info["updates"] == 0 and info["workgroups"] >= 1
    v, moved = moved_scene(sc, amplitude)
    device.update_vertices(v)
    got = device.read_bvh()
    assert np.array_equal(bits(got), bits(moved.arrays["bvh"])), describe_mismatch(got, moved.arrays["bvh"])
    assert device.refit_info()["updates"] == 1 and device.last_kernel_ms() > 0.0
    # the same vertices again: tight boxes of flat triangles — the fold's, whatever the uploaded ones were
    device.update_vertices(sc.arrays["vertices"])
    assert np.array_equal(bits(device.read_bvh()), bits(refit_ref.refit(sc.arrays["bvh"], sc.arrays["facesV"], sc.arrays["vertices"])))


@pytest.mark.parametrize("amplitude", refit_ref.AMPLITUDES)
@pytest.mark.parametrize("name", PARITY)
def test_parity_with_the_oracle_on_the_moved_scene(pbr, oracle, device, name, amplitude):
    """Upload S, update to V': whole images (.w included), the debug image, the counters and 4096 single rays equal the
    oracle's on S' — pbr_render, pbr_render_frame, pbr_render_dof with a focus point, pbr_render_adaptive."""
    sc = refit_scenes.load(pbr, name)
    v, moved = moved_scene(sc, amplitude)
    seeds = pbr.frame_seeds(0, 3)
    device.upload_scene(sc.desc)
    device.configure(sc.cfg)
    device.render(0, seeds, sc.px, sc.cam)                           # the tuner, the tile costs and the dealing orders see the old scene
    device.update_vertices(v)

    ref = oracle.Renderer(moved.desc, moved.cfg, threads=8)
    want = ref.render(0, seeds, sc.px, sc.cam)
    got = rendered(device, sc, seeds)
    assert_same_render(got, (want, ref.debug, ref.counter_dict()), "pbr_render")

    rays = rays_for(v)
    t, face, normal, counts = device.diag_trace(rays)
    want_t, want_face, want_normal, want_counts = oracle.trace_rays(moved.desc, moved.cfg, rays)
    hit = np.isfinite(want_t)
    assert hit.sum() > 500
    assert same_values(t, want_t) and np.array_equal(counts, want_counts) and np.array_equal(face[hit], want_face[hit])
    assert same_values(normal[hit], want_normal[hit])

    # frame by frame, then the same frames with a focus point through pbr_render_dof
    device.reset_accum()
    ref = oracle.Renderer(moved.desc, moved.cfg, threads=8)
    for k, seed in enumerate(seeds[:2]):
        weight = float(np.float32(k) / np.float32(k + 1))
        ref.image = ref.render_frame(float(seed), weight, sc.px, sc.cam)
        device.render_frame(float(seed), weight, sc.px, sc.cam)
        assert same_values(device.read_output(), ref.image), "pbr_render_frame %d" % k
        device.accumulate()
    cam = pbr.Camera.from_buffer_copy(sc.cam)
    cam.focusPoint[0], cam.focusPoint[1] = sc.cfg.width // 2, sc.cfg.height // 2
    ref = oracle.Renderer(moved.desc, moved.cfg, threads=8)
    want = ref.render(0, seeds, sc.px, cam)
    device.reset_accum()
    device.render_dof(0, seeds, sc.px, cam)
    assert same_values(device.read_output(), want), "pbr_render_dof: " + describe_mismatch(device.read_output(), want)

    # adaptive sampling with min = max frames never tests a tile away: pbr_render's image
    want = oracle.Renderer(moved.desc, moved.cfg, threads=8).render(0, seeds, sc.px, sc.cam)
    device.reset_accum()
    device.render_adaptive(0, seeds, sc.px, sc.cam, len(seeds), 1, len(seeds), 0.0)
    assert same_values(device.read_output(), want), "pbr_render_adaptive"
    assert (device.tile_stats()[0] == len(seeds)).all()


@pytest.mark.parametrize("amplitude", refit_ref.AMPLITUDES)
@pytest.mark.parametrize("name", ("ref_suzanne_sa_shadow", "sponza_small", "hairball_small"))
def test_updated_context_equals_fresh_upload(pbr, device, other, name, amplitude):
    """The contract: upload( S ) + update( V' ) in one context, upload( S' ) with the nodes pbr_read_bvh returns in another —
    identical images, debug images, counters, single rays, denoised images and adaptive tile statistics, with pinned plans
    and with the tuner free."""
    sc = refit_scenes.load(pbr, name)
    v, _ = moved_scene(sc, amplitude, seed=9)
    seeds = pbr.frame_seeds(0, 4)
    device.upload_scene(sc.desc)
    device.configure(sc.cfg)
    device.render(0, seeds, sc.px, sc.cam)
    device.update_vertices(v)
    fresh = sc.moved(v, device.read_bvh())
    other.upload_scene(fresh.desc)
    other.configure(sc.cfg)
    for plan in (0, 3, 4, 6, -1, -1):
        device.pin_plan(plan)
        other.pin_plan(plan)
        assert_same_render(rendered(device, sc, seeds), rendered(other, sc, seeds), "plan %d" % plan)
    rays = rays_for(v, 2048)
    for a, b in zip(device.diag_trace(rays), other.diag_trace(rays)):
        assert same_values(a, b)
    a, fa = device.denoise(sc.px, sc.cam, features=True)
    b, fb = other.denoise(sc.px, sc.cam, features=True)
    assert same_values(a, b) and same_values(fa, fb)
    for dev in (device, other):
        dev.reset_accum()
        dev.render_adaptive(0, seeds, sc.px, sc.cam, 2, 1, len(seeds), 0.05)
    assert same_values(device.read_output(), other.read_output())
    for a, b in zip(device.tile_stats(), other.tile_stats()):
        assert same_values(a, b)


def test_two_updates_equal_one_and_back_again(pbr, device, other):
    """V' then V'' == V'' alone; back to V == a fresh upload of S with the refitted boxes."""
    sc = refit_scenes.load(pbr, "ref_suzanne_schlick")
    a = sc.arrays
    v1, _ = moved_scene(sc, "large", seed=1)
    v2, moved2 = moved_scene(sc, "small", seed=2)
    for dev in (device, other):
        dev.upload_scene(sc.desc)
        dev.configure(sc.cfg)
    device.update_vertices(v1)
    device.update_vertices(v2)
    other.update_vertices(v2)
    assert np.array_equal(bits(device.read_bvh()), bits(other.read_bvh()))
    assert np.array_equal(bits(device.read_bvh()), bits(moved2.arrays["bvh"]))
    assert_same_render(rendered(device, sc), rendered(other, sc), "V' V'' against V''")
    device.update_vertices(a["vertices"])
    back = sc.moved(a["vertices"], refit_ref.refit(a["bvh"], a["facesV"], a["vertices"]))
    assert np.array_equal(bits(device.read_bvh()), bits(back.arrays["bvh"]))
    other.upload_scene(back.desc)
    assert_same_render(rendered(device, sc), rendered(other, sc), "back to V")


@pytest.mark.parametrize("traversal", (2, 3))
def test_ordered_walk_configured_after_an_update(pbr, oracle, device, other, traversal):
    """upload, update, configure( eight orders / compact ) == fresh upload of S' + the same configure == the oracle's walk over
    S'; a second update in that mode is refused with a message and changes nothing; after the reference walk is configured
    again it works."""
    sc = refit_scenes.load(pbr, "ref_suzanne_sa")
    v, moved = moved_scene(sc, "large", seed=4)
    ordered, plain = sc.config(traversal=traversal), sc.config(traversal=0)
    device.upload_scene(sc.desc)
    device.configure(plain)
    device.update_vertices(v)
    device.configure(ordered)
    other.upload_scene(moved.desc)
    other.configure(ordered)
    got = rendered(device, sc)
    assert_same_render(got, rendered(other, sc), "traversal %d" % traversal)
    ref = oracle.Renderer(moved.desc, ordered, threads=8)
    want = ref.render(0, sc.seeds, sc.px, sc.cam)
    assert_same_render(got, (want, ref.debug, ref.counter_dict()), "traversal %d against the oracle" % traversal)
    v2, moved2 = moved_scene(sc, "small", seed=6)
    with pytest.raises(pbr.PbrError, match="-3: .*ray-ordered traversal"):
        device.update_vertices(v2)
    assert_same_render(rendered(device, sc), got, "after the refusal")
    assert np.array_equal(bits(device.read_bvh()), bits(moved.arrays["bvh"]))
    device.configure(plain)
    device.update_vertices(v2)
    other.upload_scene(moved2.desc)
    other.configure(plain)
    assert_same_render(rendered(device, sc), rendered(other, sc), "reference walk again")
    device.configure(ordered)                                        # and the ordered walk is rebuilt from the newest boxes
    other.configure(ordered)
    assert_same_render(rendered(device, sc), rendered(other, sc), "traversal %d after the second update" % traversal)


def test_refusals_leave_the_context_as_it_was(pbr, device):
    sc = refit_scenes.load(pbr, "ref_suzanne_sa")
    v = sc.arrays["vertices"]
    moved, _ = moved_scene(sc, "small")
    with pytest.raises(pbr.PbrError, match="-3: .*before pbr_upload_scene"):
        device.update_vertices(v)
    count = ctypes.c_uint32()
    assert pbr.hip.pbr_read_bvh(device._ctx, None, 0, ctypes.byref(count)) == -3
    device.upload_scene(sc.desc)
    device.configure(sc.cfg)
    before = rendered(device, sc)
    nodes = device.read_bvh()

    def unchanged(what):
        assert_same_render(rendered(device, sc), before, what)
        assert np.array_equal(bits(device.read_bvh()), bits(nodes)) and device.refit_info()["updates"] == 0

    assert pbr.hip.pbr_update_vertices(device._ctx, None, v.shape[0]) == -1
    unchanged("null vertices")
    with pytest.raises(pbr.PbrError, match="-1: .*%d vertices" % (v.shape[0] - 1)):
        device.update_vertices(v[:-1])
    unchanged("another count")
    for bad in (np.inf, np.nan):
        w = moved.copy()
        w[v.shape[0] // 2, 2] = bad
        with pytest.raises(pbr.PbrError, match="-1: .*vertex %d is not finite" % (v.shape[0] // 2)):
            device.update_vertices(w)
        unchanged("a coordinate that is not finite")
    assert pbr.hip.pbr_read_bvh(device._ctx, nodes.ctypes.data, nodes.shape[0] - 1, ctypes.byref(count)) == -1 and count.value == nodes.shape[0]
    device.configure(sc.config(traversal=1))
    ordered = rendered(device, sc)
    with pytest.raises(pbr.PbrError, match="-3: .*ray-ordered traversal"):
        device.update_vertices(moved)
    assert_same_render(rendered(device, sc), ordered, "ordered traversal")
    device.configure(sc.config(phong_tessellation=0.6))
    smooth = rendered(device, sc)
    with pytest.raises(pbr.PbrError, match="-3: .*Phong tessellation"):
        device.update_vertices(moved)
    assert_same_render(rendered(device, sc), smooth, "Phong tessellation")
    assert device.refit_info()["updates"] == 0
    # after an update Phong tessellation cannot be configured until the next upload
    device.configure(sc.cfg)
    device.update_vertices(moved)
    after = rendered(device, sc)
    with pytest.raises(pbr.PbrError, match="-3: .*Phong tessellation after pbr_update_vertices"):
        device.configure(sc.config(phong_tessellation=0.6))
    assert_same_render(rendered(device, sc), after, "refused configure")
    device.upload_scene(sc.desc)
    device.configure(sc.config(phong_tessellation=0.6))
    assert_same_render(rendered(device, sc), smooth, "a new upload takes Phong tessellation again")


def test_tree_that_is_not_nested_uploads_but_cannot_be_refitted(pbr, device):
    desc, keep = hand_tree(pbr, NOT_NESTED)
    sc = keep[0]
    cfg, cam, px = sc.config(32, 32), sc.camera(), pbr.pixel_dimension(32, 32)
    device.upload_scene(desc)
    device.configure(cfg)
    info = device.refit_info()
    assert not info["nested"] and "past its parent" in info["why"] and info["device_bytes"] == 0
    device.render(0, pbr.frame_seeds(0, 2), px, cam)
    before = device.read_output()
    with pytest.raises(pbr.PbrError, match="-3: .*not properly nested .*past its parent"):
        device.update_vertices(sc.arrays()["vertices"])
    device.reset_accum()
    device.render(0, pbr.frame_seeds(0, 2), px, cam)
    assert same_values(device.read_output(), before)
    assert np.array_equal(bits(device.read_bvh()), bits(keep[1]))


def test_native_arithmetic_updated_equals_fresh(pbr, device, other):
    """arith = native: both contexts run the same kernels over the same buffers, so equality is expected (the statistical
    contract is only against the oracle)."""
    if pbr.hip.pbr_mode_built(0, 1) != 1:
        pytest.fail("this build has no native-arithmetic kernels")
    sc = refit_scenes.load(pbr, "ref_spheres_sa")
    v, moved = moved_scene(sc, "large", seed=8)
    cfg = sc.config(arith=1)
    device.upload_scene(sc.desc)
    device.configure(cfg)
    device.update_vertices(v)
    other.upload_scene(moved.desc)
    other.configure(cfg)
    for plan in (1, 4, -1):
        device.pin_plan(plan)
        other.pin_plan(plan)
        assert_same_render(rendered(device, sc), rendered(other, sc), "native, plan %d" % plan)


def test_tile_shards_after_an_update(pbr, device, gpu_device):
    """tile_world = 4 on one device: each rank's tiles after an update are the unsharded image's."""
    sc = refit_scenes.load(pbr, "ref_pillars_schlick")
    v, moved = moved_scene(sc, "large", seed=5)
    device.upload_scene(moved.desc)
    device.configure(sc.cfg)
    full = rendered(device, sc)[0]
    w, h = sc.cfg.width, sc.cfg.height
    for rank in range(4):
        dev = pbr.Device(gpu_device)
        dev.upload_scene(sc.desc)
        dev.configure(sc.config(tile_world=4, tile_rank=rank))
        dev.update_vertices(v)
        part = rendered(dev, sc)[0]
        mask = pbr.tiles.rows_of_rank(w, h, 4, rank)
        assert same_values(part[mask], full[mask]) and not part[~mask].any()
        dev.close()


def test_chunked_launches_after_an_update(pbr, device, other):
    """chunk_frames = 2: several launch pairs follow an update."""
    sc = refit_scenes.load(pbr, "sponza_small")
    v, moved = moved_scene(sc, "small", seed=7)
    seeds = pbr.frame_seeds(0, 7)
    device.set_knob("chunk_frames", 2)
    device.upload_scene(sc.desc)
    device.configure(sc.cfg)
    device.update_vertices(v)
    other.upload_scene(moved.desc)
    other.configure(sc.cfg)
    got = rendered(device, sc, seeds)
    assert device.last_trace()[1] >= 4
    assert_same_render(got, rendered(other, sc, seeds), "chunked")


def test_a_large_scene(pbr, device, other):
    """800 000 triangles: thousands of subtrees (a subtree of at most 256 nodes holds some 170 on average, so 300 000 triangles
    give fewer than 2000), a top part of several levels.  pbr_read_bvh against the numpy fold, one 256 x 256 image against a
    fresh upload."""
    sc = refit_scenes.generated(pbr, "dragon", 4, 800000, 256, 256, **{"render.max_depth": 3})
    a = sc.arrays
    assert a["facesV"].shape[0] >= 200000
    device.upload_scene(sc.desc)
    device.configure(sc.cfg)
    info = device.refit_info()
    assert info["nested"] and info["subtrees"] >= 2000 and info["top_levels"] > 1, info
    for amplitude in refit_ref.AMPLITUDES:
        v, moved = moved_scene(sc, amplitude, seed=11)
        device.update_vertices(v)
        got = device.read_bvh()
        assert np.array_equal(bits(got), bits(moved.arrays["bvh"])), describe_mismatch(got, moved.arrays["bvh"])
    other.upload_scene(moved.desc)
    other.configure(sc.cfg)
    device.pin_plan(4)
    other.pin_plan(4)
    assert_same_render(rendered(device, sc), rendered(other, sc), "large scene")


def test_multi_driver_and_path_tracer_forward_the_update(pbr, oracle, gpu_device):
    """pbr_multi_update_vertices on two contexts of one device (peer copies) and PathTracer::updateVertices: the image of S'."""
    from importlib import import_module
    multi = import_module(pbr.__name__ + ".multi")
    sc = refit_scenes.load(pbr, "ref_pillars_sa")
    v, moved = moved_scene(sc, "small", seed=12)
    want = oracle.Renderer(moved.desc, moved.cfg, threads=8).render(0, sc.seeds, sc.px, sc.cam)
    m = multi.MultiDevice([gpu_device, gpu_device], multi.PEER_COPY)
    m.upload_scene(sc.desc)
    m.configure(sc.cfg)
    m.update_vertices(v)
    m.render(0, sc.seeds, sc.px, sc.cam)
    assert same_values(m.read_full(0), want)
    with pytest.raises(pbr.PbrError):
        m.update_vertices(v[:-1])
    m.close()
    # the host driver: its frames of the moved Cornell box against a context driven by hand
    pbr.cfg_reset()
    scene = pbr.HostScene.generate("cornell")
    arrays = scene.arrays()
    moved_v = refit_ref.deform(arrays["facesV"], arrays["vertices"], "small", seed=13)
    pt = pbr.PathTracer(gpu_device, 32, 32)
    pt.initOpenCLBuffers(scene)
    pt.updateVertices(moved_v)
    assert pt.sampleCount() == 0
    got = pt.generateImages(2)
    dev = pbr.Device(gpu_device)
    dev.upload_scene(scene.desc)
    dev.configure(scene.config(32, 32))
    dev.update_vertices(moved_v)
    cam = pbr.Camera()
    pbr.host.pbrh_pt_camera(pt._h, ctypes.byref(cam))
    dev.render(0, pbr.frame_seeds(0, 2), pbr.pixel_dimension(32, 32), cam)
    assert same_values(got, dev.read_output())
    dev.close()
    pt.close()
