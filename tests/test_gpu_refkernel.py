"""The device against the reference's own kernel text as a compiler read it — no restatement in the loop: this file reads
the recorded outputs of the compiled reference kernel (tests/golden/refkernel_*.npz, tests/golden/make_refkernel.py) and
the inputs they were made from (fixtures already committed, tests/hand_scenes.py), never the CPU restatement of the kernel,
the reference or a binary built from it.

In the reference's walk (traversal 0) everything is owed bit for bit: image with its .w, debug image, and the counters
against the per-frame sums of the reference's debug images, in one plan of each kernel family.  The ray-ordered walks
(traversal 1 - 3) visit other nodes, so their counts are their own, and they owe the reference's image what SURVEY.md
section 8(c) states (tests/test_walk_order_cpu.py): only exact ties of the closest hit may differ — |d| <= 1e-4 per channel on
>= 99.5 % of the pixels and mean |d| <= 1e-5 — and every closest hit within 1e-6 max( 1, t )."""
import os
import sys

import numpy as np
import pytest

from conftest import same_values, describe_mismatch
import refit_scenes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_refkernel as mk              # noqa: E402
import make_reference_scenes as mrs      # noqa: E402

pytestmark = pytest.mark.gpu

CASE_NAMES = sorted(mk.CASES)
RAY_CASES = [n for n in CASE_NAMES if mk.CASES[n].get("rays")]
FAMILIES = ("refill-lean", "phased-mid", "phased-dual")          # one plan of each kernel family


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def scene_of(pbr, name):
    data = mk.case_inputs(name)
    _, cfg, cam, keep = mrs.scene_from_fixture(pbr, data)
    sc = refit_scenes.Scene(pbr, {k: keep[k] for k in mk.WIRE}, cfg, cam, float(data["px_dim"]), np.asarray(data["seeds"], np.float32))
    return sc, data


def render(dev, sc, data, name):
    """A fresh accumulation of the case's frames -> (image, debug image, counters added); cases with a focus point go through
    pbr_render_dof."""
    dev.reset_accum()
    before = dev.counters()
    if "focus" in mk.CASES[name]:
        dev.render_dof(data["first"], sc.seeds, sc.px, sc.cam)
    else:
        dev.render(data["first"], sc.seeds, sc.px, sc.cam)
    after = dev.counters()
    return dev.read_output(), dev.read_debug(), {k: after[k] - before[k] for k in after}


def counters_of(rec, cfg):
    """What the reference's debug images say the frames cost: their sums (recorded per frame), and one path per sample."""
    frames = rec["frame_counts"].astype(np.int64)
    return {"nodes": int(frames[:, 0].sum()), "tris": int(frames[:, 1].sum()), "paths": int(cfg.width) * int(cfg.height) * int(cfg.samples) * frames.shape[0]}


def pin(pbr, dev, plan):
    dev.pin_plan(pbr.Device.PLAN_NAMES.index(plan))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_renders_equal_the_compiled_reference_kernel(pbr, device, name):
    sc, data = scene_of(pbr, name)
    rec = mk.recorded(name)
    device.upload_scene(sc.desc)
    device.configure(sc.config(traversal=0))
    want = counters_of(rec, sc.cfg)
    for plan in FAMILIES:
        pin(pbr, device, plan)
        image, debug, counted = render(device, sc, data, name)
        assert device.last_plan()[0] == ("refill-lean-phong" if sc.cfg.phong_tessellation > 0.0 else plan)      # Phong tessellation has one plan
        assert same_values(image, rec["image"]), "%s, %s image: %s" % (name, plan, describe_mismatch(image, rec["image"]))
        assert same_values(debug, rec["debug"]), "%s, %s debug image: %s" % (name, plan, describe_mismatch(debug, rec["debug"]))
        assert {k: counted[k] for k in want} == want, "%s, %s" % (name, plan)
    a = rec["image"].astype(np.float64)[..., :3]
    for traversal, plan in zip((1, 2, 3), FAMILIES):
        device.configure(sc.config(traversal=traversal))
        pin(pbr, device, plan)
        image, _, counted = render(device, sc, data, name)
        with np.errstate(invalid="ignore"):
            d = np.abs(a - image[..., :3])
        d[np.isnan(a) & np.isnan(image[..., :3])] = 0.0
        print("%s traversal %d: %d pixels differ, max |d| %.3g" % (name, traversal, int((d.max(axis=2) > 0).sum()), d.max()))
        assert (d.max(axis=2) <= 1e-4).mean() >= 0.995 and d.mean() <= 1e-5, "%s, traversal %d" % (name, traversal)
        assert counted["paths"] == want["paths"]
    assert device.guard_trips() == [0, 0, 0]


@pytest.mark.parametrize("name", RAY_CASES)
def test_single_rays_equal_the_compiled_reference_kernel(pbr, device, name):
    sc, data = scene_of(pbr, name)
    rec = mk.recorded(name)
    rays, hit = data["rays"], np.isfinite(rec["ray_t"])
    assert rays.shape[0] == mk.RAYS and hit.sum() >= mk.RAYS // 8
    device.upload_scene(sc.desc)
    device.configure(sc.config(traversal=0))
    t, face, normal, counts = device.diag_trace(rays)
    assert same_values(t, rec["ray_t"]), "%s t: %s" % (name, describe_mismatch(t, rec["ray_t"]))
    assert np.array_equal(counts, rec["ray_counts"]), "%s: the counts of %d rays differ" % (name, (counts != rec["ray_counts"]).any(axis=1).sum())
    assert np.array_equal(face[hit], rec["ray_face"][hit]) and same_values(normal[hit], rec["ray_normal"][hit]), name
    orb = ~hit & (rec["ray_face"] < 0)                         # a ray that ends on an orb light: t = inf, the light's index
    assert np.array_equal(face[orb], rec["ray_face"][orb]), name
    for traversal in (1, 2, 3):
        device.configure(sc.config(traversal=traversal))
        t1 = device.diag_trace(rays)[0]
        assert np.array_equal(np.isfinite(t1), hit), "%s, traversal %d" % (name, traversal)
        assert np.all(np.abs(t1[hit].astype(np.float64) - rec["ray_t"][hit]) <= 1e-6 * np.maximum(1.0, rec["ray_t"][hit])), "%s, traversal %d" % (name, traversal)
    assert device.guard_trips() == [0, 0, 0]


def test_this_file_stands_on_recorded_data_alone():
    """No CPU restatement of the kernel, no reference, no binary: what is compared against comes out of tests/golden/."""
    with open(os.path.abspath(__file__)) as f:
        text = f.read()
    mentions = [line for line in text.splitlines() if line.startswith(("import ", "from ")) or " import " in line.split("#")[0]]
    assert not any("oracle" in line for line in mentions), mentions
    for name in CASE_NAMES:
        assert os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refkernel_%s.npz" % name))
