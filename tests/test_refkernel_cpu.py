"""The oracle against the reference's own kernel text as a compiler reads it (oracle/refkernel.py), with no tolerance and no
excluded pixel.

Everywhere: oracle/pt_oracle.c reproduces every recorded output of the compiled reference kernel
(tests/golden/refkernel_*.npz: frames, debug image, per-frame counter sums, single rays), and each case's "feature reached"
evidence holds on the recorded data.  Where the reference's tree exists: the binaries are built and run afresh and must
equal both the recordings and the oracle.  The builtin shim, the one place where this repository's text stands between the
reference's and the compiler, is held to the table of oracle/pt_oracle.c operation by operation."""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import same_values, describe_mismatch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_refkernel as mk              # noqa: E402
import make_reference_scenes as mrs      # noqa: E402
from oracle import refkernel             # noqa: E402

CASE_NAMES = sorted(mk.CASES)
needs_reference = pytest.mark.skipif(not refkernel.available(), reason="the reference's kernel sources only exist in the build container")
_oracle_outputs = {}


def oracle_outputs(pbr, oracle, name):
    """What oracle/pt_oracle.c makes of a case, in the recorded arrays' names; computed once."""
    if name not in _oracle_outputs:
        data = mk.case_inputs(name)
        desc, cfg, cam, keep = mrs.scene_from_fixture(pbr, data)
        r = oracle.Renderer(desc, cfg, threads=8)
        counts = []
        for k, seed in enumerate(data["seeds"]):
            n = data["first"] + k
            before = r.counter_dict()
            r.image = r.render_frame(float(seed), float(np.float32(n) / np.float32(n + 1)), float(data["px_dim"]), cam)
            after = r.counter_dict()
            counts.append([after["nodes"] - before["nodes"], after["tris"] - before["tris"]])
        out = {"image": r.image, "debug": r.debug, "frame_counts": np.array(counts, np.uint32)}
        if data["rays"].shape[0]:
            out["ray_t"], out["ray_face"], out["ray_normal"], out["ray_counts"] = oracle.trace_rays(desc, cfg, data["rays"])
        if data["lights"].shape[0]:
            out["orb_pixels"] = np.int64((oracle.trace_rays(desc, cfg, mk.centre_rays(data))[1] < 0).sum())
            rays, dist = mk.light_rays(data)
            lit = oracle.trace_rays(desc, cfg, rays)
            out["light_census"] = mk.light_census(dist, lit[0], lit[1])
        _oracle_outputs[name] = out
    return _oracle_outputs[name]


def assert_same_outputs(got, want, what):
    compared = [k for k in want if not k.startswith("values_")]
    assert sorted(compared) == sorted(k for k in got if not k.startswith("values_")), what
    for k in compared:
        assert np.shape(got[k]) == np.shape(want[k]), "%s %s" % (what, k)
        assert same_values(got[k], want[k]), "%s %s: %s" % (what, k, describe_mismatch(got[k], want[k]))


def test_the_case_table_covers_what_it_is_there_for():
    """Both BRDFs plain on every shipped scene, shadow rays, Phong 0.6 and 1.0, samples 2 and 3, depth of field on a hit and on
    a miss over four frames, depth 1, added depth 0, anti-aliasing 0 and 1.5, a first sample count above 0, two hand trees."""
    sets = [mk.CASES[n].get("set", {}) for n in CASE_NAMES]
    config = {n: dict(zip(mrs.CONFIG_FIELDS, mk.case_inputs(n)["config"])) for n in CASE_NAMES}
    assert len([n for n in CASE_NAMES if n.startswith("plain_")]) == 14
    for brdf in (0, 1):
        mine = [c for c in config.values() if c["brdf"] == brdf]
        assert {0.0, 0.6, 1.0} <= {round(float(c["phong_tessellation"]), 6) for c in mine}
        assert any(c["shadow_rays"] == 1 for c in mine) and any(c["max_depth"] == 1 and c["max_added_depth"] == 0 for c in mine)
        assert {0, 5} <= {int(c["max_added_depth"]) for c in mine}
    assert {2, 3} <= {s.get("samples") for s in sets} and {0.0, 1.5} <= {s.get("anti_aliasing") for s in sets}
    assert {e[1] for n in CASE_NAMES for e in mk.REACH[n] if e[0] == "focus"} == {"hit", "miss"}
    assert all(mk.CASES[n]["frames"] >= 3 for n in CASE_NAMES if "focus" in mk.CASES[n])
    assert any(mk.CASES[n].get("first", 0) > 0 for n in CASE_NAMES)
    nodes = {n: mk.case_inputs(n)["bvh"].shape[0] for n in CASE_NAMES if "hand" in mk.CASES[n]}
    assert min(nodes.values()) == 2 and max(nodes.values()) > 300
    assert all(mk.case_inputs(n)["rays"].shape == (mk.RAYS, 6) for n in CASE_NAMES if mk.CASES[n].get("rays"))
    assert any(("orb",) in mk.REACH[n] for n in CASE_NAMES)
    for brdf in ("sa", "schlick"):
        assert ("shadows",) in mk.REACH["plain_suzanne_%s_shadow" % brdf] and config["plain_suzanne_%s_shadow" % brdf]["shadow_rays"] == 1


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_oracle_reproduces_the_recorded_reference_kernel(pbr, oracle, name):
    assert_same_outputs(oracle_outputs(pbr, oracle, name), mk.recorded(name), name)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_each_case_reached_its_code_in_the_recorded_data(name):
    assert mk.reach_failures(name, mk.recorded) == []
    rec = mk.recorded(name)
    data = mk.case_inputs(name)
    assert dict(zip(rec["values_keys"].tolist(), rec["values_values"].tolist())) == mk.values_of(data)
    assert (rec["frame_counts"] > 0).all() and rec["frame_counts"].shape == (len(data["seeds"]), 2)
    if "orb_pixels" in rec:
        assert 0 <= int(rec["orb_pixels"]) < rec["image"].shape[0] * rec["image"].shape[1]


@needs_reference
def test_the_compiled_reference_equals_the_recordings_and_the_oracle(pbr, oracle, tmp_path):
    """One build of every configuration, one child process per case."""
    assert refkernel.build_many([mk.values_of(mk.case_inputs(n)) for n in CASE_NAMES]) is not None
    fresh = {}
    for name in CASE_NAMES:
        fresh[name] = mk.reference_outputs(name, str(tmp_path))
        assert_same_outputs(fresh[name], mk.recorded(name), name + " against the recording")
        assert_same_outputs(oracle_outputs(pbr, oracle, name), fresh[name], name + ", the oracle against a fresh run")
    for name in CASE_NAMES:
        assert mk.reach_failures(name, fresh.__getitem__) == []
    assert os.listdir(str(tmp_path)) == []


def test_values_that_do_not_survive_the_formatting_are_refused():
    base = dict(width=64, height=48, brdf=1, shadow_rays=0, max_depth=3, max_added_depth=5, samples=1, anti_aliasing=0.7,
                phong_tessellation=0.0, sky_light=[1.0, 1.0, 1.0, 0.0], num_nodes=2, num_lights=0)
    v = refkernel.config_of(**base)
    assert v["ANTI_ALIASING"] == "0.700000f" and v["PHONGTESS"] == "0" and v["SKY_LIGHT"] == "(float4)( 1.000000, 1.000000, 1.000000, 0.0f )"
    assert refkernel.config_of(**dict(base, phong_tessellation=0.6))["PHONGTESS"] == "1"
    for bad in (dict(anti_aliasing=0.1234567), dict(phong_tessellation=1.0 / 3.0), dict(sky_light=[0.8460001, 1.0, 1.0, 0.0])):
        with pytest.raises(ValueError):
            refkernel.config_of(**dict(base, **bad))
    assert refkernel.key_of(v) != refkernel.key_of(dict(v, BVH_NUM_NODES="3"))


# ---- the shim against the table ---------------------------------------------------------------------------------------

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
SUB = F(1e-41)
BELOW_ONE = F(float.fromhex("0x1.fffffep-1"))
EDGES = np.array([0.0, -0.0, 1.0, -1.0, INF, -INF, NAN, SUB, -SUB, F(1.17549435e-38), F(3.4028235e38), 0.5, -2.5, 1e-20, 3.0], np.float32)


def round32(x):
    """A Fraction rounded to binary32, nearest-even, subnormals included."""
    c = F(float(x))
    if not np.isfinite(c):
        big = Fraction(float(F(3.4028235e38))) + Fraction(2) ** 103        # half an ulp above the largest: beyond it, inf
        return c if abs(x) >= big else F(np.sign(float(x))) * F(3.4028235e38)
    best = c
    for other in (np.nextafter(c, -INF), np.nextafter(c, INF)):
        if np.isfinite(other):
            d0, d1 = abs(Fraction(float(best)) - x), abs(Fraction(float(other)) - x)
            if d1 < d0 or (d1 == d0 and (other.view(np.uint32) & 1) == 0 and (best.view(np.uint32) & 1) == 1):
                best = other
    return best


def fma32(a, b, c):
    """fmaf: one rounding.  Non-finite operands or results go through float64, where nothing is lost that matters to them."""
    a, b, c = F(a), F(b), F(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return F(np.float64(a) * np.float64(b) + np.float64(c))
    return round32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def dot32(a, b):
    with np.errstate(all="ignore"):
        return fma32(a[2], b[2], fma32(a[1], b[1], F(a[0]) * F(b[0])))


def cross32(a, b):
    with np.errstate(all="ignore"):
        return np.array([fma32(a[1], b[2], -(F(a[2]) * F(b[1]))), fma32(a[2], b[0], -(F(a[0]) * F(b[2]))), fma32(a[0], b[1], -(F(a[1]) * F(b[0])))], np.float32)


def min32(a, b):
    """C's fminf / fmaxf as the oracle uses them: the other operand where one is NaN."""
    return np.fmin(F(a), F(b))


@pytest.fixture(scope="module")
def shim(tmp_path_factory, oracle):
    if refkernel.clang() is None:
        pytest.skip("no clang++ for the shim's vector types")
    lib = ctypes.CDLL(refkernel.build_shim(str(tmp_path_factory.mktemp("shim"))))
    fp = ctypes.POINTER(ctypes.c_float)
    lib.rk_shim_probe.argtypes = [ctypes.c_int, fp, ctypes.c_int, fp]
    lib.rk_shim_probe.restype = None

    def probe(op, items):
        items = np.ascontiguousarray(items, np.float32).reshape(-1, 12)
        out = np.empty((items.shape[0], 4), np.float32)
        lib.rk_shim_probe(op, items.ctypes.data_as(fp), items.shape[0], out.ctypes.data_as(fp))
        return out
    return probe


def operands(columns, n=384, seed=3):
    """(n + edge rows, 12): random values over many magnitudes, then rows drawn from EDGES in every column used."""
    rng = np.random.default_rng(seed)
    rnd = (rng.normal(size=(n, 12)) * 10.0 ** rng.integers(-6, 7, (n, 12))).astype(np.float32)
    edge = EDGES[rng.integers(0, EDGES.size, (256, 12))]
    edge[: EDGES.size, :] = EDGES[:, None]                       # every edge value in every column at once ...
    mixed = np.where(rng.random((256, 12)) < 0.4, edge, rnd[:256])       # ... and edges among ordinary values
    out = np.concatenate([rnd, edge, mixed]).astype(np.float32)
    out[:, columns:] = 0.0
    return out


SCALAR_OPS = {  # op: (operand columns, numpy float32 restatement of the table's line)
    0: (1, lambda p: F(1.0) / p[0]), 2: (2, lambda p: p[0] / p[1]), 3: (1, lambda p: np.sqrt(p[0])),
    11: (2, lambda p: np.fmin(p[0], p[1])), 12: (2, lambda p: np.fmax(p[0], p[1])), 15: (1, lambda p: np.abs(p[0])),
    17: (2, lambda p: p[1] if p[0] < p[1] else p[0]), 18: (3, lambda p: np.fmin(np.fmax(p[0], p[1]), p[2])),
}


@pytest.mark.parametrize("op", sorted(SCALAR_OPS))
def test_shim_scalar_builtins_follow_the_table(shim, op):
    columns, line = SCALAR_OPS[op]
    items = operands(columns)
    got = shim(op, items)[:, 0]
    with np.errstate(all="ignore"):
        want = np.array([line(p) for p in items], np.float32)
    assert same_values(got, want), describe_mismatch(got, want)
    both_zero = (got == 0) & (want == 0)
    if op in (0, 2, 3, 15):             # the sign of a zero is part of these lines (fmin( -0, +0 ) may be either)
        assert np.array_equal(np.signbit(got[both_zero]), np.signbit(want[both_zero]))


def test_shim_fract_follows_the_table(shim):
    items = operands(1)
    items[:8, 0] = [0.0, -0.0, -1e-10, 1.0, 43758.5453123, -43758.5, 16777216.0, -0.5]
    got = shim(9, items)[:, :2]
    with np.errstate(all="ignore"):
        whole = np.floor(items[:, 0])
        want = np.stack([np.fmin(items[:, 0] - whole, BELOW_ONE), whole], axis=1)
    assert same_values(got, want), describe_mismatch(got, want)
    assert got[2, 0] == BELOW_ONE                       # -1e-10 - floor = 1 in binary32: the clamp below one is what answers


def test_shim_vector_builtins_follow_the_table(shim):
    items = operands(9)
    with np.errstate(all="ignore"):
        a, b, c = items[:, 0:3], items[:, 3:6], items[:, 6:9]
        want = {
            1: F(1.0) / a, 13: np.fmin(a, b), 14: np.fmax(a, b), 16: np.abs(a),
            4: np.array([dot32(x, y) for x, y in zip(a, b)], np.float32)[:, None],
            5: np.array([cross32(x, y) for x, y in zip(a, b)], np.float32),
            8: np.array([[fma32(x[k], y[k], z[k]) for k in range(3)] for x, y, z in zip(a, b, c)], np.float32),
        }
        squared = np.array([dot32(x, x) for x in a], np.float32)
        want[7] = np.sqrt(squared)[:, None]
        want[6] = a * (F(1.0) / np.sqrt(squared))[:, None]
    for op, w in sorted(want.items()):
        got = shim(op, items)[:, : w.shape[1]]
        assert same_values(got, w), "op %d: %s" % (op, describe_mismatch(got, w))


def test_shim_float4_builtins_follow_the_table(shim):
    items = operands(9)
    with np.errstate(all="ignore"):
        x, y, a = items[:, 0:4], items[:, 4:8], items[:, 8:9]
        mix = x + (y - x) * a
        lo, hi = items[:, 4:5], items[:, 5:6]
        clamp = np.fmin(np.fmax(x, lo), hi)
    assert same_values(shim(10, items), mix), describe_mismatch(shim(10, items), mix)
    assert same_values(shim(19, items), clamp), describe_mismatch(shim(19, items), clamp)


@pytest.mark.parametrize("op,name", [(20, "sin"), (21, "cos"), (22, "tan"), (23, "acos"), (24, "atan"), (25, "pow"), (26, "cbrt")])
def test_shim_transcendentals_are_the_oracles(shim, oracle, op, name):
    items = operands(2)
    if name == "acos":
        items[:384, 0] = np.linspace(-1.0, 1.0, 384, dtype=np.float32)
    if name == "pow":
        items[:384, 0] = np.abs(items[:384, 0])
        items[:384, 1] = np.random.default_rng(5).uniform(-8, 8, 384).astype(np.float32)
        items[:8, 1] = [0.0, 1.0, 2.0, 3.0, 100000.0, 0.1666666666, -1.0, 0.5]
    got = shim(op, items)[:, 0]
    want = oracle.math(name, items[:, 0], items[:, 1])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) or same_values(got, want), describe_mismatch(got, want)


def test_round32_is_a_correct_rounding():
    """The yardstick of the fused operations, against cases with known answers."""
    assert round32(Fraction(1) + Fraction(1, 2 ** 24)) == F(1.0)                              # tie to even
    assert round32(Fraction(1) + Fraction(3, 2 ** 24)) == F(1.0) + F(2.0 ** -22)              # tie to even, upwards
    assert round32(Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)) == np.nextafter(F(1.0), INF)      # float64 would round this to the tie first
    assert round32(Fraction(1, 2 ** 149) * Fraction(3, 2)) == F(2.0 ** -148)                  # subnormal tie
    assert fma32(F(4.0), F(1e38), F(0.0)) == INF and np.isnan(fma32(INF, F(0.0), F(1.0)))
