"""The HIP kernels' Phong-tessellation stages (pbr_diag_math "cbrt", pbr_diag_solve_cubic, pbr_diag_phong_face) and the
Phong build of the walk (pbr_diag_trace with phong_tessellation configured) against float64, in both arithmetics.

Exact arithmetic: the three hooks are the oracle's bit for bit on every committed batch, and — with no oracle in the loop —
pass the float64 assertions of test_phong_ref_cpu.py at the same bounds.

Native arithmetic (pbr_config.arith = PBR_ARITH_NATIVE; the hooks follow the context's configuration): cbrt as in the exact
arithmetic (binary64 in both); solveCubic and the patch against float64 with the same hard invariants, the same 1e-3
tolerance in t, the same 0.5 % and 10 % caps and the same angle bound; K_CUBIC and the median bounds times NATIVE_SCALE =
32 (test_gpu_shading_ref.py gives the reason: the worst native operation is 32 roundings of the one rounding per operation
the exact bounds are multiples of).  These native bounds were set before any GPU run, and held on the first one.

MEASURED on the MI355X (the batches of test_phong_ref_cpu.py, 4096 items each):
  exact    every figure of test_phong_ref_cpu.py's table again, digit for digit — the hooks are the oracle's bit for bit.
  native   cbrt 0.49999992 ulp (the same bits).  solveCubic: every clear count right, worst |root - true| / ( 2^-23 ( cond +
           |r| ) ) = 791.4 (a0 = 10.2, a1 = 1073, a2 = 298, a3 = 0.578) against 32 x 512; median 0.079.
           patches (ambiguous shares as in the exact table: they belong to the reference):
             batch        failures          median rel t   worst angle  median angle
             random 0.3   0.10 % (1 + 3)    1.12e-7        2.58e-3      2.29e-7
             random 0.6   0                 8.84e-8        8.21e-4      2.20e-7
             random 1.0   0.05 % (2 + 0)    7.89e-8        2.92e-3      2.33e-7
             curved       0                 7.00e-8        3.30e-3      2.50e-7
             axis         0                 7.90e-8        3.52e-4      1.82e-7
             tNear < 0    0.02 % (0 + 1)    8.63e-8        2.54e-3      2.17e-7
             interval     0                 9.24e-8        2.66e-5      2.64e-7
           no hit the reference lacks; nearly flat and through-the-origin batches as in the exact arithmetic (74.3 % and
           67.9 % of the clear cases fail, no NaN).
  walk     400 rays, 2340 ( ray, curved face ) cases, 378 hits in float64, 3.5 % of the rays ambiguous, no failure; median
           relative error in t 3.3e-8, worst 4.8e-6.

The walk: the ball on the floor of test_gpu_parity.smooth_scene at alpha = 0.6, 400 rays aimed at it.  pbr_diag_trace is
orc_trace_rays bit for bit in traversals 0 - 3, counters included, and in traversal 0 agrees with brute force in float64
over ALL faces with no tree walk: a curved face through phong_ref.patch_hits, clipped to [ |tNear|, tFar ] of the leaf box
that holds it (the slab interval in float64 from the uploaded node array; a ray that misses that box never meets the
face), a flat face through Moeller-Trumbore; the same tolerance and caps as for the patch batches.
"""
import numpy as np
import pytest

import phong_ref as pr
from conftest import same_values, describe_mismatch
from test_gpu_parity import smooth_scene
from test_gpu_shading_ref import NATIVE_SCALE, configure
from test_phong_ref_cpu import (AMBIGUOUS_MAX, BATCHES, FAIL_MAX, K_CUBIC, T_TOL, Stages, batch_items, cubic_reference, run_cbrt,
                                run_cubic, run_patch_batch, run_recorded_batch)

pytestmark = pytest.mark.gpu

REGULAR = ["random 0.3", "random 0.6", "random 1.0", "curved", "axis", "tnear", "interval"]
RECORDED = ["flat", "origin"]


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def device_stages(pbr, dev, arith=0):
    """The device as the stages under test.  Exact: a fresh context, no scene, no configuration — the hooks need neither.
    Native: the context configured with arith = native."""
    if arith:
        configure(pbr, dev, 1, arith)
    return Stages(lambda x: dev.diag_math("cbrt", x), dev.diag_solve_cubic, dev.diag_phong_face, NATIVE_SCALE if arith else 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# exact arithmetic
# ---------------------------------------------------------------------------------------------------------------------

def test_exact_hooks_are_the_oracles_bit_for_bit(pbr, oracle, device):
    x = pr.cbrt_inputs()
    got, want = device.diag_math("cbrt", x), oracle.math("cbrt", x)
    assert same_values(got, want), describe_mismatch(got, want)
    c = cubic_reference()[0]
    got, want = device.diag_solve_cubic(c), oracle.solve_cubic(c)
    assert same_values(got, want), describe_mismatch(got, want)
    for name in BATCHES:
        items = batch_items(name)
        got, want = device.diag_phong_face(items), oracle.phong_face(items)
        assert same_values(got, want), name + ": " + describe_mismatch(got, want)
    # ... and stay so in a context that was configured for the exact arithmetic
    configure(pbr, device, 1, 0)
    items = batch_items("curved")
    assert same_values(device.diag_phong_face(items), oracle.phong_face(items))


def test_hooks_follow_the_configured_arithmetic(pbr, oracle, device):
    items, c = batch_items("curved"), cubic_reference()[0]
    configure(pbr, device, 1, 1)
    assert not same_values(device.diag_phong_face(items), oracle.phong_face(items))
    assert not same_values(device.diag_solve_cubic(c), oracle.solve_cubic(c))
    x = pr.cbrt_inputs()[: 1 << 16]
    assert same_values(device.diag_math("cbrt", x), oracle.math("cbrt", x))       # binary64 in both arithmetics


def test_exact_cbrt_within_one_ulp_of_float64(pbr, device):
    run_cbrt(device_stages(pbr, device))


def test_exact_solve_cubic_against_float64_roots(pbr, device):
    run_cubic(device_stages(pbr, device), K_CUBIC)


@pytest.mark.parametrize("name", REGULAR)
def test_exact_patch_intersection_against_float64(pbr, device, name):
    run_patch_batch(device_stages(pbr, device), name)


@pytest.mark.parametrize("name", RECORDED)
def test_exact_nearly_flat_and_through_the_origin_hold_the_hard_invariants(pbr, device, name):
    run_recorded_batch(device_stages(pbr, device), name)


# ---------------------------------------------------------------------------------------------------------------------
# native arithmetic
# ---------------------------------------------------------------------------------------------------------------------

def test_native_cbrt_within_one_ulp_of_float64(pbr, device):
    run_cbrt(device_stages(pbr, device, 1))


def test_native_solve_cubic_against_float64_roots(pbr, device):
    run_cubic(device_stages(pbr, device, 1), NATIVE_SCALE * K_CUBIC)


@pytest.mark.parametrize("name", REGULAR)
def test_native_patch_intersection_against_float64(pbr, device, name):
    run_patch_batch(device_stages(pbr, device, 1), name)


@pytest.mark.parametrize("name", RECORDED)
def test_native_nearly_flat_and_through_the_origin_hold_the_hard_invariants(pbr, device, name):
    run_recorded_batch(device_stages(pbr, device, 1), name)


# ---------------------------------------------------------------------------------------------------------------------
# the walk
# ---------------------------------------------------------------------------------------------------------------------

def ball_rays(n=400):
    """Rays from 3 - 4.5 units away, above the floor, towards points of the ball (radius 0.6 about ( 0, 0.75, 0 )) and, a
    quarter of them, of the floor around it."""
    rng = np.random.default_rng(77)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 1] = np.abs(d[:, 1]) * 0.8 + 0.05
    origin = np.array([0.0, 0.75, 0.0]) + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(3.0, 4.5, (n, 1))
    target = np.array([0.0, 0.75, 0.0]) + rng.uniform(-0.62, 0.62, (n, 3))
    floor = rng.random(n) < 0.25
    target[floor] = np.stack([rng.uniform(-1.9, 1.9, floor.sum()), np.zeros(floor.sum()), rng.uniform(-1.9, 1.9, floor.sum())], axis=1)
    rays = np.zeros((n, 6), np.float32)
    rays[:, 0:3] = origin
    rays[:, 3:6] = target - origin
    rays[:, 3:6] /= np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1, keepdims=True)
    return rays


def brute_force(arr, rays, alpha):
    """(t, ambiguous) per ray in float64 over all faces (module docstring)."""
    n = rays.shape[0]
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    v = arr["vertices"][:, :3].astype(np.float64)
    fv = arr["facesV"][:, :3].astype(np.int64)
    tri_n = arr["normals"][:, :3].astype(np.float64)[arr["facesN"][:, :3].astype(np.int64)]
    curved = ~(np.all(tri_n[:, 0] == tri_n[:, 1], axis=1) & np.all(tri_n[:, 1] == tri_n[:, 2], axis=1))
    best = np.full(n, np.inf)
    ambiguous = np.zeros(n, bool)

    # flat faces: Moeller-Trumbore
    flat = np.flatnonzero(~curved)
    a, e1, e2 = v[fv[flat, 0]], v[fv[flat, 1]] - v[fv[flat, 0]], v[fv[flat, 2]] - v[fv[flat, 0]]
    for k in range(n):
        p = np.cross(d[k], e2)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / (e1 * p).sum(1)
            tv = o[k] - a
            uu = (tv * p).sum(1) * inv
            q = np.cross(tv, e1)
            vv = (q * d[k]).sum(1) * inv
            tt = (e2 * q).sum(1) * inv
        inside = np.minimum(np.minimum(uu, vv), 1.0 - uu - vv)
        ok = (inside >= 0) & (tt > 1e-4) & np.isfinite(tt)
        ambiguous[k] |= bool((np.isfinite(tt) & (tt > 0) & (np.abs(inside) < pr.EDGE_TOL)).any())
        if ok.any():
            best[k] = tt[ok].min()

    # curved faces: per leaf the slab interval, per ( ray, face of a leaf the ray meets ) a patch case
    bvh = arr["bvh"].astype(np.float64)
    leaves = np.flatnonzero(bvh[:, 3] >= 0)
    leaves = leaves[leaves >= 1]                                   # node 0 is the root container, never tested
    cases = []
    for leaf in leaves:
        t_near, t_far = pr._slab(bvh[leaf, 0:3], bvh[leaf, 4:7], o, d)
        met = np.flatnonzero((t_near <= t_far) & (t_far > 1e-5))
        for face in (int(bvh[leaf, 3]), int(bvh[leaf, 7])):
            if face >= 0 and curved[face]:
                cases += [(k, face, t_near[k], t_far[k]) for k in met]
    ray_of = np.array([c[0] for c in cases])
    face_of = np.array([c[1] for c in cases])
    items = np.zeros((len(cases), 32), np.float32)
    items[:, 0:9] = v[fv[face_of]].reshape(-1, 9)
    items[:, 9:18] = tri_n[face_of].reshape(-1, 9)
    items[:, 18:24] = rays[ray_of]
    items[:, 24], items[:, 25], items[:, 26], items[:, 27] = np.inf, [c[2] for c in cases], [c[3] for c in cases], alpha
    ref = pr.reference(items)
    np.minimum.at(best, ray_of, ref["t"])
    np.logical_or.at(ambiguous, ray_of, ref["amb"])
    return best, ambiguous, len(cases)


@pytest.mark.parametrize("traversal", [0, 1, 2, 3])
def test_phong_walk_is_the_oracles_and_agrees_with_brute_force(pbr, oracle, device, tmp_path, traversal):
    sc = smooth_scene(pbr, tmp_path, **{"render.phong_tessellation": 0.6})
    assert sc.desc.num_lights == 0
    cfg = sc.config(64, 48)
    cfg.traversal = traversal
    assert cfg.phong_tessellation == np.float32(0.6)
    rays = ball_rays()
    device.upload_scene(sc.desc)
    device.configure(cfg)
    t, face, normal, counts = device.diag_trace(rays)
    ot, oface, onormal, ocounts = oracle.trace_rays(sc.desc, cfg, rays)
    assert same_values(t, ot), describe_mismatch(t, ot)
    hit = np.isfinite(ot)
    assert hit.sum() > 200
    assert np.array_equal(face[hit], oface[hit]) and same_values(normal, onormal), describe_mismatch(normal, onormal)
    assert np.array_equal(counts, ocounts)
    assert device.guard_trips() == [0, 0, 0]
    # the hook follows the configuration: the same rays with the tessellation off hit flat triangles
    flat = sc.config(64, 48)
    flat.traversal = traversal
    flat.phong_tessellation = 0.0
    device.configure(flat)
    ft, _, fnormal, _ = device.diag_trace(rays)
    assert not same_values(ft, t) and not same_values(fnormal, normal)

    if traversal != 0:
        return
    arr = sc.arrays()
    want, ambiguous, cases = brute_force(arr, rays, float(np.float32(0.6)))
    clear = ~ambiguous
    got = t.astype(np.float64)
    wrong_kind = clear & (np.isfinite(got) != np.isfinite(want))
    both = clear & np.isfinite(got) & np.isfinite(want)
    rel = np.abs(got[both] - want[both]) / np.maximum(1.0, want[both])
    fails = int(wrong_kind.sum()) + int((rel > T_TOL).sum())
    print("walk: %d rays, %d ( ray, curved face ) cases, %d hits in float64, ambiguous %.2f %%, failures %d (%d hit / miss, %d beyond 1e-3), rel t median %.3g max %.3g"
          % (len(rays), cases, int(np.isfinite(want).sum()), 100 * ambiguous.mean(), fails, int(wrong_kind.sum()), int((rel > T_TOL).sum()),
             float(np.median(rel)), float(rel.max())))
    assert np.isfinite(want).sum() > 200
    assert ambiguous.mean() <= AMBIGUOUS_MAX
    assert fails <= FAIL_MAX * clear.sum()
