"""The walks INSIDE the render kernels — pathTracing, pathTracingPhased and pathTracingDual, every plan, the reference walk and the
three ray-ordered ones, in the exact and in the native arithmetic — held per pixel to a float64 brute force over all faces,
closest hit and any hit.  No diagnostic entry point: the production render calls are the probe (tests/walk_truth.py): with
max_depth = 1 an image's .w is the camera ray's closest hit and its rgb tells hit from miss exactly; with max_depth = 2, a
black sky, shadow rays and one point light a pixel is lit exactly where the shadow walk found the light.
tests/test_walk_truth_cpu.py holds what is assumed here about the inputs — cameras, lights, margins, the oracle's zero
exceptions, planted defects caught.  The margins (EDGE_MARGIN exact, NATIVE_SCALE * EDGE_MARGIN native) are input conditions.

64 x 48, two frames; per (case, arithmetic, BRDF) one upload, traversals 0 - 3 x two probes x seven plans.

MEASURED (records, not thresholds) — the largest |w - t64| / max( 1, t64 ) over the decided pixels of every render of a leg,
the decided share, and the sizes of the black and the lit set:
                       exact: error  decided  black  lit   native: error  decided  black  lit
  wide7      BRDF 1     4.26e-07  100.0 %   2332   636      4.36e-07   99.8 %   2325   635
  wide40     BRDF 1     5.67e-07   99.8 %   2392   504      3.83e-07   99.5 %   2384   502
  wide40     BRDF 0     5.67e-07   99.8 %   2392   521      3.83e-07   99.5 %   2384   519
  chain300   BRDF 1     6.57e-07   99.8 %   2043   936      1.47e-06   99.0 %   2022   925
  cut257     BRDF 1     5.91e-07   99.7 %   2107   870      7.29e-07   99.3 %   2099   862
  cornell    BRDF 1     1.82e-07   98.4 %   2505   508      1.68e-07   98.2 %   2502   506
  cornell    BRDF 0     1.82e-07   98.4 %   2505   509      1.68e-07   98.2 %   2502   507
  sponza-6k  BRDF 1     3.75e-07   99.9 %   1520  1315      3.75e-07   99.0 %   1496  1303
  wide40 frame by frame: the figures of wide40, BRDF 1, in both arithmetics
(of 3072 pixels; the black set counts the decided misses too).  The exact figures are the oracle's own, bit for bit; the native
walk stays within a few binary32 roundings of them, three orders of magnitude inside the tolerance 1e-3 max( 1, t ).
"""
import numpy as np
import pytest

import walk_truth as wt
from test_gpu_parity import PLANS
from test_walk_truth_cpu import MARGINS, assert_probe_a, assert_probe_b
from test_gpu_shading_ref import K_NATIVE

pytestmark = pytest.mark.gpu

TRAVERSALS = (0, 1, 2, 3)
ARITH = {"exact": 0, "native": 1}


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def needs_modes(pbr, arith, traversals):
    """A build may leave the native flavours out (pbr_mode_built); the exact ones are the product."""
    missing = [t for t in traversals if pbr.hip.pbr_mode_built(t, arith) != 1]
    if missing and arith == 1:
        pytest.skip("the native flavour of traversal(s) %s is not in this build (pbr_mode_built)" % missing)
    assert not missing, missing


def flavour(traversal, arith):
    """The namespace of a mode's kernels (csrc/pt_flavour.hpp): bit 0 a ray-ordered walk, bit 1 native, bit 2 compact records."""
    return "ptk_f%d::" % ((1 if traversal else 0) | (2 if arith else 0) | (4 if traversal == 3 else 0))


def check_a(device, image, first, mask, what):
    """Probe A on one render: no outlier, exact colours, .w finite or +inf everywhere, every path and every hit counted."""
    worst = assert_probe_a(image, first, mask, what)
    w = image[..., 3]
    finite = np.isfinite(w)
    assert (finite | np.isposinf(w)).all(), what
    counters = device.counters()
    assert counters["paths"] == wt.W * wt.H * wt.FRAMES and counters["hits"] == int(finite.sum()) * wt.FRAMES, (what, counters, int(finite.sum()))
    return worst


def check_b(image, first, black, lit, what):
    assert_probe_b(image, first, black, lit, what)
    rgb = image[..., :3]                                     # (.w is the first-hit distance: inf on a miss)
    assert np.isfinite(rgb).all(), (what, "not finite", np.argwhere(~np.isfinite(rgb))[:4].tolist())


def report(name, arith, brdf, worst, mask, black, lit):
    print("%s, %s, BRDF %d: largest |w - t64| / max( 1, t64 ) = %.3g; %.1f %% decided, black set %d, lit set %d" % (
        name, arith, brdf, worst, 100 * mask.mean(), black.sum(), lit.sum()))


@pytest.mark.parametrize("arith", sorted(ARITH))
@pytest.mark.parametrize("name", wt.CASES)
def test_render_kernels_walk_to_the_float64_truth(pbr, device, name, arith):
    needs_modes(pbr, ARITH[arith], TRAVERSALS)
    for brdf in wt.BRDFS[name]:
        sc, first, shadow, gate = wt.truth(pbr, name, brdf, K_NATIVE)
        mask, black, lit = wt.sets(first, shadow, gate, MARGINS[ARITH[arith]])
        device.upload_scene(sc.desc)
        worst, kernels = 0.0, set()
        for traversal in TRAVERSALS:
            for probe, config in (("A", wt.config_a), ("B", wt.config_b)):
                device.configure(config(sc, brdf, traversal=traversal, arith=ARITH[arith]))
                for plan in PLANS:
                    what = (name, arith, brdf, traversal, probe, plan)
                    device.pin_plan(PLANS[plan])
                    device.reset_accum()
                    device.render(0, sc.seeds, sc.px, sc.cam)
                    assert device.last_plan()[0] == plan and device.last_kernel().startswith(flavour(traversal, ARITH[arith])), (what, device.last_kernel())
                    kernels.add(device.last_kernel().split("::")[1].split("<")[0])
                    image = device.read_output()
                    if probe == "A":
                        worst = max(worst, check_a(device, image, first, mask, what))
                    else:
                        check_b(image, first, black, lit, what)
        report(name, arith, brdf, worst, mask, black, lit)
        assert kernels == {"pathTracing", "pathTracingPhased", "pathTracingDual"}, kernels        # the three families, in this mode
    assert device.guard_trips() == [0, 0, 0]


@pytest.mark.parametrize("arith", sorted(ARITH))
def test_single_frame_launches_walk_to_the_float64_truth(pbr, device, arith):
    """render_frame + accumulate, two frames, on wide40: the launch shape of one frame, traversals 0 and 3."""
    needs_modes(pbr, ARITH[arith], (0, 3))
    name, brdf = "wide40", 1
    sc, first, shadow, gate = wt.truth(pbr, name, brdf, K_NATIVE)
    mask, black, lit = wt.sets(first, shadow, gate, MARGINS[ARITH[arith]])
    device.upload_scene(sc.desc)
    worst = 0.0
    for traversal in (0, 3):
        for probe, config in (("A", wt.config_a), ("B", wt.config_b)):
            what = (name, arith, brdf, traversal, probe, "frame by frame")
            device.configure(config(sc, brdf, traversal=traversal, arith=ARITH[arith]))
            device.reset_accum()
            for k, seed in enumerate(sc.seeds):
                if k:
                    device.accumulate()
                device.render_frame(float(seed), float(np.float32(k) / np.float32(k + 1)), sc.px, sc.cam)
            image = device.read_output()
            assert device.last_kernel().startswith(flavour(traversal, ARITH[arith])), (what, device.last_kernel())
            if probe == "A":
                worst = max(worst, check_a(device, image, first, mask, what))
            else:
                check_b(image, first, black, lit, what)
    report(name + " frame by frame", arith, brdf, worst, mask, black, lit)
    assert device.guard_trips() == [0, 0, 0]
