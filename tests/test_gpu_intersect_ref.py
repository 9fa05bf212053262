"""The HIP kernels' primitives of the walk (pbr_diag_intersect: triangleT on the uploaded face record, boxHit<false> and
boxHit<true> with the walk's inverse direction, intersectSphere) in both arithmetics.

Exact arithmetic: the random batches and the edge sets of test_intersect_ref_cpu.py equal the oracle's hook bit for bit and
pass the float64 check (tests/intersect_ref.py) at K_EXACT, the dyadic verdicts included.

Native arithmetic (pbr_config.arith = PBR_ARITH_NATIVE: `/` as v_rcp_f32 without correction steps, v_sqrt_f32, the
inverse direction by v_rcp_f32): the same cases at the project's native bounds, fixed before any run — K_NATIVE = 32 K_EXACT,
NATIVE_SCALE times the median and the ambiguous share, subnormal intermediates flushed — with the hard invariant that nothing
is non-finite where the float64 reference is finite and bounded.  The dyadic verdicts are not asserted there: either
branch counts.

One test holds the three new stages (camera ray, intersection, surface step) to the configured arithmetic."""
import numpy as np
import pytest

from conftest import describe_mismatch, same_values
from test_camera_ref_cpu import Setup, random_items
from test_gpu_shading_ref import K_NATIVE, NATIVE_SCALE, configure
from test_intersect_ref_cpu import OPS, RANDOM, Prims, run_edges, run_random
from test_shading_ref_cpu import AMBIGUOUS_MAX, K_EXACT, MEDIAN_MAX, random_surface

pytestmark = pytest.mark.gpu


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def device_prims(pbr, dev, arith, oracle=None):
    """The device as the implementation under test; with an oracle, every batch must equal its hook bit for bit."""
    configure(pbr, dev, 1, arith)

    def fn(op, items):
        got = dev.diag_intersect(op, items)
        if oracle is not None:
            want = oracle.intersect(op, items)
            assert same_values(got, want), "%s: %s" % (op, describe_mismatch(got, want))
        return got

    if arith == 0:
        return Prims(fn)
    return Prims(fn, NATIVE_SCALE * MEDIAN_MAX, NATIVE_SCALE * AMBIGUOUS_MAX, flush=True, exact=False)


@pytest.mark.parametrize("op", OPS)
def test_exact_mode_random_batches_equal_the_oracle_and_match_float64(pbr, oracle, device, op):
    run_random(device_prims(pbr, device, 0, oracle), op, K_EXACT, seed=1)


@pytest.mark.parametrize("op", OPS)
def test_exact_mode_edge_set_equals_the_oracle_and_matches_float64(pbr, oracle, device, op):
    run_edges(device_prims(pbr, device, 0, oracle), op, K_EXACT)


@pytest.mark.parametrize("op", OPS)
def test_native_mode_random_batches_match_float64(pbr, device, op):
    run_random(device_prims(pbr, device, 1), op, K_NATIVE, seed=2)


@pytest.mark.parametrize("op", OPS)
def test_native_mode_edge_set_matches_float64(pbr, device, op):
    run_edges(device_prims(pbr, device, 1), op, K_NATIVE)


def test_new_stages_follow_the_configured_arithmetic(pbr, oracle, device):
    """No configuration: the oracle's bits where a stage needs none (the primitives), PBR_ESTATE where it needs one (the camera
    ray: width, height and anti-aliasing are the configuration's).  Exact configuration: the oracle's bits.  Native: other
    bits.  Exact again: the oracle's bits again."""
    rng = np.random.default_rng(12)
    mtl = np.asarray([1, 1.5, 200.0, 20.0, 0.5, 0.5, 0, 0, .5, .5, .5, 0, 1, 1, 1, 0], np.float32)
    setup = Setup(64, 48, 1.5, (0.25, 2.0))
    cam_items = random_items(rng, setup, 1024)
    tri = RANDOM["triangle"](rng, 1024)
    box = RANDOM["box"](rng, 1024)
    sph = RANDOM["sphere"](rng, 1024)
    surf = random_surface(rng, 1024, lambda x: oracle.math("randhash", x))
    want = {
        "camera": oracle.camera_ray(setup.width, setup.height, setup.anti_aliasing, setup.struct(oracle.OrcCamera), setup.px_dim, cam_items),
        "triangle": oracle.intersect("triangle", tri), "box": oracle.intersect("box", box), "sphere": oracle.intersect("sphere", sph),
        "surface": oracle.surface_step(1, mtl, surf),
    }

    for op, items in (("triangle", tri), ("box", box), ("sphere", sph)):
        got = device.diag_intersect(op, items)                       # a fresh context: nothing uploaded, nothing configured
        assert same_values(got, want[op]), "%s, no configuration: %s" % (op, describe_mismatch(got, want[op]))
    with pytest.raises(Exception, match="configure"):
        device.diag_camera_ray(setup.px_dim, setup.struct(pbr.Camera), cam_items)

    def run(arith):
        sc, _, keep = configure(pbr, device, 1, arith, mtl)
        cfg = sc.config(setup.width, setup.height)
        cfg.anti_aliasing, cfg.arith = setup.anti_aliasing, arith
        device.configure(cfg)
        return {
            "camera": device.diag_camera_ray(setup.px_dim, setup.struct(pbr.Camera), cam_items),
            "triangle": device.diag_intersect("triangle", tri), "box": device.diag_intersect("box", box),
            "sphere": device.diag_intersect("sphere", sph), "surface": device.diag_surface_step(surf),
        }

    for arith, equal in ((0, True), (1, False), (0, True)):
        got = run(arith)
        for name in want:
            assert same_values(got[name], want[name]) == equal, "%s, arith %d: %s" % (name, arith, describe_mismatch(got[name], want[name]))
