"""The HIP kernels' camera ray (pbr_diag_camera_ray: initRay with the host's launch-invariant camera terms, the
anti-aliasing jitter and the depth-of-field lens) in both arithmetics.

Exact arithmetic: the random batches and the edge sets of test_camera_ref_cpu.py equal the oracle's hook bit for bit and
pass the float64 check (tests/camera_ref.py) at K_EXACT.

Native arithmetic (normalisations by v_rsq_f32, v_sin_f32 / v_cos_f32 in the jitter and the lens, v_sqrt_f32): the same
cases at the project's native bounds, fixed before any run — K_NATIVE = 32 K_EXACT, NATIVE_SCALE times the median and the
ambiguous share, subnormal intermediates flushed — with the hard invariant that nothing is non-finite where the float64
reference is finite and bounded.  The draws are the device's own (pbr_diag_math "randhash" in the arithmetic under test);
the seeds whose first draw is 0 or next to 1 are found in the exact hash."""
import pytest

from conftest import describe_mismatch, same_values
from test_camera_ref_cpu import Cameras, run_edges, run_random
from test_gpu_parity import make_scene
from test_gpu_shading_ref import K_NATIVE, NATIVE_SCALE
from test_shading_ref_cpu import AMBIGUOUS_MAX, K_EXACT, MEDIAN_MAX

pytestmark = pytest.mark.gpu


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def device_cameras(pbr, dev, arith, oracle=None):
    """The device as the implementation under test; with an oracle, every batch must equal its hook bit for bit."""
    sc = make_scene(pbr)
    dev.upload_scene(sc.desc)
    state = {}

    def use(setup):
        key = (setup.width, setup.height, setup.anti_aliasing)
        if state.get("key") != key:
            cfg = sc.config(setup.width, setup.height)
            cfg.anti_aliasing, cfg.arith = setup.anti_aliasing, arith
            dev.configure(cfg)
            state["key"] = key

    def fn(setup, items):
        use(setup)
        got = dev.diag_camera_ray(setup.px_dim, setup.struct(pbr.Camera), items)
        if oracle is not None:
            want = oracle.camera_ray(setup.width, setup.height, setup.anti_aliasing, setup.struct(oracle.OrcCamera), setup.px_dim, items)
            assert same_values(got, want), describe_mismatch(got, want)
        return got

    def randhash(x):                      # called after fn: the context is configured by then
        return dev.diag_math("randhash", x)

    if arith == 0:
        return Cameras(fn, randhash)
    return Cameras(fn, randhash, NATIVE_SCALE * MEDIAN_MAX, NATIVE_SCALE * AMBIGUOUS_MAX, flush=True)


def test_exact_mode_random_batches_equal_the_oracle_and_match_float64(pbr, oracle, device):
    run_random(device_cameras(pbr, device, 0, oracle), K_EXACT, seed=1)


def test_exact_mode_edge_set_equals_the_oracle_and_matches_float64(pbr, oracle, device):
    run_edges(device_cameras(pbr, device, 0, oracle), K_EXACT, lambda x: oracle.math("randhash", x))


def test_native_mode_random_batches_match_float64(pbr, device):
    top = run_random(device_cameras(pbr, device, 1), K_NATIVE, seed=2)
    print("native camera ray, random batches: largest error / bound %.3g of K_NATIVE = %d" % (top, K_NATIVE))


def test_native_mode_edge_set_matches_float64(pbr, oracle, device):
    top = run_edges(device_cameras(pbr, device, 1), K_NATIVE, lambda x: oracle.math("randhash", x))
    print("native camera ray, edge sets: largest error / bound %.3g of K_NATIVE = %d" % (top, K_NATIVE))
