"""pbr_update_geometry on the GPU: the thick boxes equal the numpy restatement (tests/patch_refit_ref.py) bit for bit, the
Phong patch records equal packScene's of the moved scene S', and an updated context behaves exactly like a fresh upload of S'
under Phong tessellation — against the oracle on S' and context against context, in the reference walk and in the ordered walks
behind the re-link; pbr_configure's state rule; every refusal leaves the context as it was."""
import ctypes

import numpy as np
import pytest

import patch_refit_ref
import refit_ref
import refit_scenes
from conftest import same_values, describe_mismatch
from test_patch_refit_cpu import smooth_scene

pytestmark = pytest.mark.gpu

ALPHA = 0.6
GEOMETRIES = ("ref_suzanne_sa", "ref_spheres_schlick", "ref_squirrels_sa", "ref_pillars_sa")


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


def with_arrays(sc, **arrays):
    a = dict(sc.arrays)
    a.update({k: np.ascontiguousarray(v, np.float32) for k, v in arrays.items()})
    return refit_scenes.Scene(sc.pbr, a, sc.cfg, sc.cam, sc.px, sc.seeds)


_moved = {}


def moved_scene(pbr, name, amplitude, alpha=ALPHA, seed=3):
    """(S, V', N', S'): the fixture, deformed positions, perturbed normals and the scene a fresh upload would take — V', N' and
    the numpy thick refit's nodes.  Computed once per case and shared; nobody writes to the arrays."""
    key = (name, amplitude, alpha, seed)
    if key not in _moved:
        sc = refit_scenes.load(pbr, name)
        a = sc.arrays
        v = refit_ref.deform(a["facesV"], a["vertices"], amplitude, seed)
        n = patch_refit_ref.perturb_normals(a["normals"], seed)
        nodes = patch_refit_ref.refit(a["bvh"], a["facesV"], a["facesN"], v, n, alpha)
        _moved[key] = (sc, v, n, with_arrays(sc, vertices=v, normals=n, bvh=nodes))
    return _moved[key]


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
def test_boxes_and_patches_equal_the_numpy_restatement(pbr, device, name, amplitude):
    """configure( phong 0.6 ), update_geometry( V', N' ): read_bvh() == patch_refit_ref.refit with the .w words untouched,
    read_patches() == packScene's triPN of S'.  normals=None keeps the patch normals; with phong 0 and on an unconfigured
    context the boxes are refit_ref.refit's — pbr_update_vertices's."""
    sc, v, n, moved = moved_scene(pbr, name, amplitude)
    a = sc.arrays
    device.upload_scene(sc.desc)
    assert device.patch_refit_info() == {"patches": True, "device_bytes": 0, "updates": 0, "last_update": False, "alpha": 0.0}
    assert np.array_equal(bits(device.read_patches()), bits(patch_refit_ref.pack_patches(a["facesV"], a["facesN"], a["vertices"], a["normals"])))
    kept = device.refit_info()["device_bytes"]
    # unconfigured: alpha is 0
    device.update_geometry(v, n)
    tight = refit_ref.refit(a["bvh"], a["facesV"], v)
    assert np.array_equal(bits(device.read_bvh()), bits(tight)), "unconfigured"
    want_patches = patch_refit_ref.pack_patches(a["facesV"], a["facesN"], v, n)
    assert np.array_equal(bits(device.read_patches()), bits(want_patches))
    faces, normals = a["facesV"].shape[0], a["normals"].shape[0]
    info = device.patch_refit_info()
    assert info == {"patches": True, "device_bytes": 40 * faces + 16 * normals, "updates": 1, "last_update": True, "alpha": 0.0}
    assert device.refit_info()["device_bytes"] == kept and device.refit_info()["updates"] == 1
    # a new upload starts over; Phong tessellation configured
    device.upload_scene(sc.desc)
    device.configure(sc.config(phong_tessellation=ALPHA))
    device.update_geometry(v, n)
    got = device.read_bvh()
    assert np.array_equal(bits(got), bits(moved.arrays["bvh"])), describe_mismatch(got, moved.arrays["bvh"])
    assert np.array_equal(bits(got[:, [3, 7]]), bits(a["bvh"][:, [3, 7]]))
    assert np.array_equal(bits(device.read_patches()), bits(want_patches))
    assert device.patch_refit_info()["alpha"] == np.float32(ALPHA) and device.last_kernel_ms() > 0.0
    # positions only: the normals of the last update stay
    device.update_geometry(a["vertices"])
    assert np.array_equal(bits(device.read_patches()), bits(patch_refit_ref.pack_patches(a["facesV"], a["facesN"], a["vertices"], n)))
    assert np.array_equal(bits(device.read_bvh()), bits(patch_refit_ref.refit(a["bvh"], a["facesV"], a["facesN"], a["vertices"], n, ALPHA)))
    assert device.patch_refit_info()["device_bytes"] == info["device_bytes"] and device.patch_refit_info()["updates"] == 2
    # positions only on a fresh upload: the uploaded normals
    device.upload_scene(sc.desc)
    device.update_geometry(v)
    assert np.array_equal(bits(device.read_patches()), bits(patch_refit_ref.pack_patches(a["facesV"], a["facesN"], v, a["normals"])))
    # phong 0 configured: tight boxes again
    device.configure(sc.config(phong_tessellation=0.0))
    device.update_geometry(v, n)
    assert np.array_equal(bits(device.read_bvh()), bits(tight)), "phong 0"


def test_alpha_one_on_suzanne(pbr, device):
    sc, v, n, moved = moved_scene(pbr, "ref_suzanne_sa", "small", alpha=1.0)
    device.upload_scene(sc.desc)
    device.configure(sc.config(phong_tessellation=1.0))
    device.update_geometry(v, n)
    got = device.read_bvh()
    assert np.array_equal(bits(got), bits(moved.arrays["bvh"])), describe_mismatch(got, moved.arrays["bvh"])


@pytest.mark.parametrize("amplitude", refit_ref.AMPLITUDES)
@pytest.mark.parametrize("name", ("ref_suzanne_sa", "ref_spheres_schlick"))
def test_parity_with_the_oracle_on_the_moved_scene(pbr, oracle, device, name, amplitude):
    """Upload S, configure Phong tessellation, update to ( V', N' ): whole images (.w included), the debug image, the counters
    and 4096 single rays equal the oracle's on S' — pbr_render, pbr_render_frame + pbr_accumulate, pbr_render_adaptive."""
    sc, v, n, moved = moved_scene(pbr, name, amplitude)
    cfg = sc.config(phong_tessellation=ALPHA)
    seeds = pbr.frame_seeds(0, 3)
    device.upload_scene(sc.desc)
    device.configure(cfg)
    device.render(0, seeds, sc.px, sc.cam)                           # the tuner, the tile costs and the dealing orders see the old scene
    device.update_geometry(v, n)

    ref = oracle.Renderer(moved.desc, cfg, threads=8)
    want = ref.render(0, seeds, sc.px, sc.cam)
    got = rendered(device, sc, seeds)
    assert_same_render(got, (want, ref.debug, ref.counter_dict()), "pbr_render")
    assert device.last_plan()[0] == "refill-lean-phong"

    rays = rays_for(v)
    t, face, normal, counts = device.diag_trace(rays)
    want_t, want_face, want_normal, want_counts = oracle.trace_rays(moved.desc, cfg, rays)
    hit = np.isfinite(want_t)
    assert hit.sum() > 500
    assert same_values(t, want_t) and np.array_equal(counts, want_counts) and np.array_equal(face[hit], want_face[hit])
    assert same_values(normal[hit], want_normal[hit])

    device.reset_accum()
    ref = oracle.Renderer(moved.desc, cfg, threads=8)
    for k, seed in enumerate(seeds[:2]):
        weight = float(np.float32(k) / np.float32(k + 1))
        ref.image = ref.render_frame(float(seed), weight, sc.px, sc.cam)
        device.render_frame(float(seed), weight, sc.px, sc.cam)
        assert same_values(device.read_output(), ref.image), "pbr_render_frame %d" % k
        device.accumulate()

    # adaptive sampling with min = max frames never tests a tile away: pbr_render's image
    device.reset_accum()
    device.render_adaptive(0, seeds, sc.px, sc.cam, len(seeds), 1, len(seeds), 0.0)
    assert same_values(device.read_output(), want), "pbr_render_adaptive"
    assert (device.tile_stats()[0] == len(seeds)).all()


@pytest.mark.parametrize("name", ("ref_suzanne_sa", "ref_squirrels_sa"))
def test_updated_context_equals_fresh_upload(pbr, device, other, name):
    """The contract, context against context: upload( S ) + configure + update_geometry( V', N' ) against upload( S' ) with the
    nodes pbr_read_bvh returns + the same configure — images, debug images, counters, single rays, the denoised image; and
    again after a second update back to ( V, N )."""
    sc, v, n, _ = moved_scene(pbr, name, "large", seed=9)
    a = sc.arrays
    cfg = sc.config(phong_tessellation=ALPHA)
    seeds = pbr.frame_seeds(0, 3)
    device.upload_scene(sc.desc)
    device.configure(cfg)
    device.render(0, seeds, sc.px, sc.cam)
    for what, vertices, normals in (("V' N'", v, n), ("back to V N", a["vertices"], a["normals"])):
        device.update_geometry(vertices, normals)
        fresh = with_arrays(sc, vertices=vertices, normals=normals, bvh=device.read_bvh())
        other.upload_scene(fresh.desc)
        other.configure(cfg)
        assert np.array_equal(bits(device.read_patches()), bits(other.read_patches()))
        assert_same_render(rendered(device, sc, seeds), rendered(other, sc, seeds), what)
        rays = rays_for(vertices, 2048)
        for x, y in zip(device.diag_trace(rays), other.diag_trace(rays)):
            assert same_values(x, y)
        x, fx = device.denoise(sc.px, sc.cam, features=True)
        y, fy = other.denoise(sc.px, sc.cam, features=True)
        assert same_values(x, y) and same_values(fx, fy)


@pytest.mark.parametrize("traversal", (1, 2, 3))
def test_ordered_walks_are_relinked_under_phong_tessellation(pbr, oracle, device, other, traversal):
    """pbr_refit_ordered_walk on, traversal t with Phong tessellation: read_walk() is byte for byte what configure( traversal 0 ),
    update_geometry, configure( t ) leaves on a second context, and the render equals the oracle's in that walk."""
    sc, v, n, moved = moved_scene(pbr, "ref_suzanne_sa", "large", seed=4)
    ordered, plain = sc.config(traversal=traversal, phong_tessellation=ALPHA), sc.config(traversal=0, phong_tessellation=ALPHA)
    device.refit_ordered_walk(True)
    device.upload_scene(sc.desc)
    device.configure(ordered)
    device.update_geometry(v, n)
    assert device.relink_info()["relinked"]
    other.upload_scene(sc.desc)
    other.configure(plain)
    other.update_geometry(v, n)
    other.configure(ordered)                                          # the state rule lets it: the last update was under 0.6
    got_walk, want_walk = device.read_walk(), other.read_walk()
    assert np.array_equal(got_walk[0], want_walk[0]) and got_walk[1:] == want_walk[1:]
    got = rendered(device, sc)
    ref = oracle.Renderer(moved.desc, ordered, threads=8)
    want = ref.render(0, sc.seeds, sc.px, sc.cam)
    assert_same_render(got, (want, ref.debug, ref.counter_dict()), "traversal %d against the oracle" % traversal)
    assert_same_render(got, rendered(other, sc), "traversal %d against the three-call sequence" % traversal)


def test_state_rule_of_configure(pbr, device):
    sc, v, n, moved = moved_scene(pbr, "ref_pillars_sa", "small")
    smooth, flat = sc.config(phong_tessellation=ALPHA), sc.config(phong_tessellation=0.0)
    device.upload_scene(sc.desc)
    device.configure(smooth)
    device.update_geometry(v, n)
    device.configure(smooth)                                          # the same alpha: allowed
    device.configure(flat)                                            # phong 0 over thick boxes: always allowed
    device.configure(smooth)                                          # ... and the boxes are still 0.6's
    before = rendered(device, sc)
    with pytest.raises(pbr.PbrError, match="-3: .*Phong tessellation"):
        device.configure(sc.config(phong_tessellation=1.0))          # another alpha
    with pytest.raises(pbr.PbrError, match="-3: .*Phong tessellation"):
        device.configure(sc.config(phong_tessellation=float(np.nextafter(np.float32(ALPHA), np.float32(1)))))
    assert_same_render(rendered(device, sc), before, "refused configure")
    # an update under phong 0 makes tight boxes: 0.6 is refused afterwards
    device.configure(flat)
    device.update_geometry(v, n)
    with pytest.raises(pbr.PbrError, match="-3: .*Phong tessellation"):
        device.configure(smooth)
    # back under 0.6 — impossible without an upload: the update needs 0.6 configured, and 0.6 cannot be configured
    device.upload_scene(sc.desc)
    device.configure(smooth)
    device.update_geometry(v, n)
    device.configure(flat)
    device.update_vertices(v)                                        # leaves the patches stale and the boxes tight
    with pytest.raises(pbr.PbrError, match="-3: .*Phong tessellation after pbr_update_vertices"):
        device.configure(smooth)
    assert not device.patch_refit_info()["last_update"]
    device.upload_scene(sc.desc)                                     # a new upload clears it
    device.configure(smooth)
    # pbr_update_vertices itself still refuses under Phong tessellation
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_vertices while Phong tessellation"):
        device.update_vertices(v)


def test_refusals_leave_the_context_as_it_was(pbr, device):
    sc, moved_v, moved_n, _ = moved_scene(pbr, "ref_suzanne_sa", "small")
    v, n = sc.arrays["vertices"], sc.arrays["normals"]
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_geometry before pbr_upload_scene"):
        device.update_geometry(v, n)
    device.upload_scene(sc.desc)
    device.configure(sc.config(phong_tessellation=ALPHA))
    before, nodes, patches = rendered(device, sc), device.read_bvh(), device.read_patches()

    def unchanged(what):
        assert_same_render(rendered(device, sc), before, what)
        assert np.array_equal(bits(device.read_bvh()), bits(nodes)) and np.array_equal(bits(device.read_patches()), bits(patches)), what
        assert device.patch_refit_info()["updates"] == 0 and device.refit_info()["updates"] == 0

    update = pbr.hip.pbr_update_geometry
    assert update(device._ctx, None, v.shape[0], n.ctypes.data, n.shape[0]) == -1
    unchanged("null vertices")
    with pytest.raises(pbr.PbrError, match="-1: .*%d vertices" % (v.shape[0] - 1)):
        device.update_geometry(moved_v[:-1], moved_n)
    unchanged("another vertex count")
    with pytest.raises(pbr.PbrError, match="-1: .*%d normals" % (n.shape[0] - 1)):
        device.update_geometry(moved_v, moved_n[:-1])
    unchanged("another normal count")
    assert update(device._ctx, moved_v.ctypes.data, v.shape[0], None, n.shape[0]) == -1
    unchanged("null normals with a count")
    assert update(device._ctx, moved_v.ctypes.data, v.shape[0], moved_n.ctypes.data, 0) == -1
    unchanged("normals with count 0")
    for bad in (np.inf, np.nan):
        w = moved_v.copy()
        w[v.shape[0] // 2, 2] = bad
        with pytest.raises(pbr.PbrError, match="-1: .*vertex %d is not finite" % (v.shape[0] // 2)):
            device.update_geometry(w, moved_n)
        unchanged("a position that is not finite")
        m = moved_n.copy()
        m[n.shape[0] // 3, 0] = bad
        with pytest.raises(pbr.PbrError, match="-1: .*normal %d is not finite" % (n.shape[0] // 3)):
            device.update_geometry(moved_v, m)
        unchanged("a normal that is not finite")
    # an ordered traversal without pbr_refit_ordered_walk
    device.configure(sc.config(traversal=2, phong_tessellation=ALPHA))
    before = rendered(device, sc)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_geometry while a ray-ordered traversal"):
        device.update_geometry(moved_v, moved_n)
    unchanged("ordered traversal")
    count = ctypes.c_uint32()
    assert pbr.hip.pbr_diag_read_patches(device._ctx, patches.ctypes.data, patches.shape[0] * 6 - 1, ctypes.byref(count)) == -1
    assert count.value == patches.shape[0] * 6


def test_scene_without_usable_normals(pbr, device):
    """Uploaded without normals (dTriPN is not there): new normals are refused with PBR_ESTATE and nothing changes; positions
    alone are taken, with pbr_update_vertices's boxes."""
    sc, v, n, _ = moved_scene(pbr, "ref_pillars_sa", "small")
    a = sc.arrays
    bare = with_arrays(sc)
    bare.desc.facesN, bare.desc.normals, bare.desc.num_normals = None, None, 0
    device.upload_scene(bare.desc)
    device.configure(sc.cfg)
    before, nodes = rendered(device, sc), device.read_bvh()
    assert not device.patch_refit_info()["patches"]
    with pytest.raises(pbr.PbrError, match="-3: .*read_patches"):
        device.read_patches()
    with pytest.raises(pbr.PbrError, match="-1: .*normals"):
        device.update_geometry(v, n)                                  # the upload's count is 0
    assert pbr.hip.pbr_update_geometry(device._ctx, v.ctypes.data, v.shape[0], n.ctypes.data, 0) == -1
    assert_same_render(rendered(device, sc), before, "refused")
    assert np.array_equal(bits(device.read_bvh()), bits(nodes)) and device.refit_info()["updates"] == 0
    device.update_geometry(v)
    assert np.array_equal(bits(device.read_bvh()), bits(refit_ref.refit(a["bvh"], a["facesV"], v)))
    assert device.patch_refit_info()["device_bytes"] == 0
    # normals there, indices out of range: the count matches, the scene has no patches — PBR_ESTATE
    broken = with_arrays(sc)
    wild = a["facesN"].copy()
    wild[0, 0] = a["normals"].shape[0]
    broken.arrays["facesN"] = wild
    broken.desc.facesN = wild.ctypes.data
    device.upload_scene(broken.desc)
    device.configure(sc.cfg)
    before, nodes = rendered(device, sc), device.read_bvh()
    with pytest.raises(pbr.PbrError, match="-3: .*without usable vertex normals"):
        device.update_geometry(v, n)
    assert_same_render(rendered(device, sc), before, "refused")
    assert np.array_equal(bits(device.read_bvh()), bits(nodes)) and device.refit_info()["updates"] == 0


def test_not_nested_tree_is_refused(pbr, device):
    from test_scene_pack_cpu import hand_tree, NOT_NESTED
    desc, keep = hand_tree(pbr, NOT_NESTED)
    device.upload_scene(desc)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_geometry: .*not properly nested"):
        device.update_geometry(keep[0].arrays()["vertices"])
    assert np.array_equal(bits(device.read_bvh()), bits(keep[1]))


def test_the_builders_boxes_on_the_device(pbr, device, tmp_path):
    """The smooth ball built by the host builder with alpha 0.6: update_geometry( V, N ) unchanged reproduces the uploaded
    nodes as float values, and the render does not change."""
    sc = smooth_scene(pbr, tmp_path, **{"render.max_depth": 4, "render.phong_tessellation": ALPHA})
    a = sc.arrays()
    pbr.cfg_set(**{"render.max_depth": 4, "render.phong_tessellation": ALPHA})
    cfg, cam, px = sc.config(32, 24), sc.camera(), pbr.pixel_dimension(32, 24)
    pbr.cfg_reset()
    assert cfg.phong_tessellation == np.float32(ALPHA)
    seeds = pbr.frame_seeds(0, 2)
    device.upload_scene(sc.desc)
    device.configure(cfg)
    device.render(0, seeds, px, cam)
    before = device.read_output(), device.read_debug(), device.counters()
    device.update_geometry(a["vertices"], a["normals"])
    got = device.read_bvh()
    assert np.array_equal(got, a["bvh"]), describe_mismatch(got, a["bvh"])
    device.reset_accum()
    device.render(0, seeds, px, cam)
    assert_same_render((device.read_output(), device.read_debug(), device.counters()), before, "unchanged geometry")
    assert device.last_plan()[0] == "refill-lean-phong"


def test_path_tracer_forwards_the_update(pbr, gpu_device, tmp_path):
    """PathTracer::updateGeometry: the tracer's frames of the moved smooth ball against a context driven by hand."""
    overrides = {"render.max_depth": 4, "render.phong_tessellation": ALPHA}
    scene = smooth_scene(pbr, tmp_path, **overrides)
    arrays = scene.arrays()
    v = refit_ref.deform(arrays["facesV"], arrays["vertices"], "small", seed=13)
    n = patch_refit_ref.perturb_normals(arrays["normals"], seed=13)
    pbr.cfg_set(**overrides)
    pt = pbr.PathTracer(gpu_device, 32, 32)
    pt.initOpenCLBuffers(scene)
    pt.updateGeometry(v, n)
    assert pt.sampleCount() == 0
    got = pt.generateImages(2)
    dev = pbr.Device(gpu_device)
    dev.upload_scene(scene.desc)
    dev.configure(scene.config(32, 32))
    pbr.cfg_reset()
    dev.update_geometry(v, n)
    cam = pbr.Camera()
    pbr.host.pbrh_pt_camera(pt._h, ctypes.byref(cam))
    dev.render(0, pbr.frame_seeds(0, 2), pbr.pixel_dimension(32, 32), cam)
    assert dev.last_plan()[0] == "refill-lean-phong"
    assert same_values(got, dev.read_output())
    dev.close()
    pt.close()
