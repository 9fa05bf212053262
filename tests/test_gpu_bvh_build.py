"""pbr_build_bvh on the GPU against its numpy restatement (tests/bvh_build_ref.py): the same tree, not merely a valid one —
node count, every .w word, facesV_out and facesN_out exactly, the boxes by value (-0.0 == +0.0: which zero fminf returns for
a mixed pair is not part of the contract) — for both builders, the clustering builder at radii 1, 3, 32 and 64, on inputs
chosen for the places where a builder goes wrong unnoticed (tests/bvh_build_cases.py); and the radius a build reports."""
import numpy as np
import pytest

import bvh_build_cases as cases
import bvh_build_ref as ref

pytestmark = pytest.mark.gpu

NAMES = list(cases.FULL) + ["%s-%d" % s for s in cases.SCENES]
CONFIGS = [("ploc", 1), ("ploc", 3), ("ploc", 32), ("ploc", 64), ("lbvh", -1)]
_inputs = {}


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def inputs(pbr, name):
    if name not in _inputs:
        if name in cases.FULL:
            _inputs[name] = cases.FULL[name]()
        else:
            kind, triangles = name.rsplit("-", 1)
            _inputs[name] = cases.scene(pbr, kind, int(triangles))
        for a in _inputs[name]:
            a.setflags(write=False)
    return _inputs[name]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_tree(got, want):
    (nodes, outV, outN), (r_nodes, r_outV, r_outN) = got, want
    assert nodes.shape == r_nodes.shape, "node count %d, restated %d" % (nodes.shape[0], r_nodes.shape[0])
    for what, a, b in (("facesV_out", outV, r_outV), ("facesN_out", outN, r_outN),
                       (".w words", bits(nodes[:, [3, 7]]), bits(r_nodes[:, [3, 7]])),
                       ("boxes", nodes[:, [0, 1, 2, 4, 5, 6]], r_nodes[:, [0, 1, 2, 4, 5, 6]])):
        assert a.shape == b.shape and a.dtype == b.dtype, what
        if not np.array_equal(a, b):
            rows = np.nonzero((a != b).any(1))[0]
            raise AssertionError("%s: %d of %d rows differ, first row %d: %r, restated %r" % (what, rows.size, a.shape[0], rows[0], a[rows[0]], b[rows[0]]))


def restated(v, fv, fn, builder, radius):
    return ref.lbvh(v, fv, fn) if builder == "lbvh" else ref.ploc(v, fv, fn, radius)


@pytest.mark.parametrize("builder,radius", CONFIGS)
@pytest.mark.parametrize("name", NAMES)
def test_device_build_equals_the_restatement(pbr, device, name, builder, radius):
    v, fv, fn = inputs(pbr, name)
    device.set_knob("bvh_builder", {"ploc": 0, "lbvh": 1}[builder])
    device.set_knob("ploc_radius", radius)
    assert_same_tree(device.build_bvh(v, fv, fn), restated(v, fv, fn, builder, radius))
    if builder == "ploc":
        assert device.bvh_build_radius() == ref.radius_used(radius, False) == radius


@pytest.mark.parametrize("name", ["soup-300", "strip-257"])
def test_a_radius_knob_above_the_limit_builds_with_64(pbr, device, name):
    v, fv, fn = inputs(pbr, name)
    device.set_knob("ploc_radius", 200)
    got = device.build_bvh(v, fv, fn)
    assert device.bvh_build_radius() == ref.radius_used(200, False) == 64
    assert_same_tree(got, ref.ploc(v, fv, fn, 64))
    device.set_knob("ploc_radius", 64)
    assert_same_tree(device.build_bvh(v, fv, fn), got)


def test_the_default_radius_follows_the_configured_traversal(pbr, device):
    """No knob: 32 on a context that is not configured or configured for the reference's walk, 3 once it is configured for
    an ordered one — and the tree is the restatement's at that radius; a knob >= 1 replaces either."""
    v, fv, fn = inputs(pbr, "soup-300")
    assert_same_tree(device.build_bvh(v, fv, fn), ref.ploc(v, fv, fn, 32))
    assert device.bvh_build_radius() == ref.radius_used(-1, False) == 32
    pbr.cfg_reset()
    sc = pbr.HostScene.generate("cornell", 1, 0)
    device.upload_scene(sc.desc)
    for traversal, ordered in ((0, False), (2, True)):
        cfg = sc.config(32, 32)
        cfg.traversal = traversal
        device.configure(cfg)
        want = ref.radius_used(-1, ordered)
        assert want == (3 if ordered else 32)
        assert_same_tree(device.build_bvh(v, fv, fn), ref.ploc(v, fv, fn, want))
        assert device.bvh_build_radius() == want
    for knob in (0, 1, 7):
        device.set_knob("ploc_radius", knob)
        want = ref.radius_used(knob, True)
        assert want == (knob if knob >= 1 else 3)
        assert_same_tree(device.build_bvh(v, fv, fn), ref.ploc(v, fv, fn, want))
        assert device.bvh_build_radius() == want
