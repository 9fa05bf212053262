"""ptd::temporalMotion and ptd::temporalIntegrate on planted histories (csrc/pt_temporal.hpp), through pbr_diag_temporal.

a. Every case of tests/temporal_planes.py — thresholds hit exactly and missed by an ulp, candidates behind the camera, off the
   scale and outside the image, histories that are not finite in one word, degenerate, mirrored and overflowing faces, images
   from 1 x 1 to 70 x 9 — gives the restatements' `integrated`, `history`, `lengths`, `motion` and `reference` with `same_values`:
   tolerance 0, the header's contract.  Where it does not, the message says per kind of pixel how far the device and the
   restatement are from the float64 truth (tests/test_temporal_planes_cpu.py holds restatement and truth together on the host).
b. pbr_diag_temporal is the public path: on a hand-made scene at 24 x 16 the second and third pbr_denoise_temporal calls — a
   camera move, then pbr_update_vertices under motion tracking — equal it on what the device returned, bit for bit.
c. It leaves the context alone, and every refusal of include/pbr_hip_diag.h is PBR_EINVAL and writes nothing.
d. Printed, not asserted: how many pixels of test_gpu_temporal.py's Cornell sequences take each decision of the class table."""
import collections
import types

import numpy as np
import pytest

import hand_scenes
import temporal_planes as T
import temporal_ref as ref
import test_temporal_planes_cpu as cpu
from conftest import same_values, describe_mismatch
from test_gpu_temporal import SEQUENCES, cornell, view
from test_gpu_temporal import step as cornell_step

pytestmark = pytest.mark.gpu

F = np.float32
PBR_EINVAL = "-1:"
CASES = [pytest.param(case, id=case.name) for case in T.cases()]
OUTPUTS = ("integrated", "history", "motion", "reference")
COUNTED = {}             # sequence name -> Counter of its decisions, for the total of (d)


@pytest.fixture(scope="module")
def planes_device(pbr, gpu_device):
    """One context for all of (a): pbr_diag_temporal needs it for its device and stream only and leaves it as it was."""
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


# ---- a: the device is the restatement, and who left the truth where it is not ------------------------------------------------

def explain(case, got):
    """Per kind of differing pixel — (candidate, valid mask, blend or copy, motion code) of the restatement's record — the
    device's and the restatement's largest distance from the float64 truth, per quantity."""
    r = T.evaluate(case)
    differs = np.zeros((case.h, case.w), bool)
    for key in OUTPUTS:
        want = getattr(r.rest, key)
        if want is not None:
            a, b = np.asarray(got[key]), np.asarray(want)
            differs |= (~((a == b) | (np.isnan(a) & np.isnan(b)))).any(-1)
    differs |= got["lengths"] != r.rest.history[..., 2]
    device = types.SimpleNamespace(integrated=got["integrated"], history=got["history"], motion=got.get("motion"), reference=got.get("reference"))
    (e_dev, _), (e_rest, _) = cpu.errors(case, device, r.truth), cpu.errors(case, r.rest, r.truth)
    rec = r.rest_record
    kinds = collections.defaultdict(list)
    for y, x in np.argwhere(differs):
        kinds[(ref.CANDIDATES[int(rec.candidate[y, x])], int(r.rest.history[y, x, 3]), ref.COPIES[int(rec.copy[y, x])],
               None if rec.code is None else int(rec.code[y, x]))].append((y, x))
    lines = ["%d pixels differ" % differs.sum()]
    for kind, where in sorted(kinds.items(), key=str):
        ys, xs = np.array(where).T
        with np.errstate(all="ignore"):
            figures = ", ".join("%s device %.3e restatement %.3e" % (q, np.nanmax(e_dev[q][ys, xs]), np.nanmax(e_rest[q][ys, xs])) for q in e_dev)
        lines.append("  %r, %d pixels, first (y, x) = %s; from the truth: %s" % (kind, len(where), where[0], figures))
    return "\n".join(lines)


@pytest.mark.parametrize("case", CASES)
def test_planted_histories_give_the_restatement_s_bits(pbr, planes_device, case):
    want = T.evaluate(case).rest
    got = planes_device.diag_temporal(**T.device_inputs(pbr, case))
    assert set(got) == {"integrated", "history", "lengths"} | ({"motion", "reference"} if case.motion is not None else set())
    same = all(same_values(got[key], getattr(want, key)) for key in OUTPUTS if getattr(want, key) is not None)
    same = same and same_values(got["lengths"], want.history[..., 2]) and got["lengths"].dtype == np.uint32
    assert same, "%s: %s" % (case.name, explain(case, got))


# ---- b: the diag entry is the public path ----------------------------------------------------------------------------------------

BW, BH, FRAMES = 24, 16, 2


def hand_scene(pbr, dev):
    sc = hand_scenes.scene(pbr, "wide40")
    dev.upload_scene(sc.desc)
    dev.configure(sc.config(width=BW, height=BH))
    px = pbr.pixel_dimension(BW, BH)
    a = sc.arrays
    cams = [hand_scenes.camera(pbr, a["vertices"], sc.flat, toward, 1.1) for toward in ((4.0, 3.0, 6.0), (4.3, 3.1, 5.8))]
    return sc, px, cams


def public_step(pbr, dev, px, cam, seed0, temporal, motion=False):
    """test_gpu_temporal's step at this size: what the call was given, read from the device, and all it returns."""
    s = cornell_step(pbr, dev, px, cam, seed0, temporal, None, FRAMES)
    if motion:
        s.motion, s.face = dev.temporal_motion()
    return s


def as_previous(s):
    return dict(integrated=s.integrated, features=np.stack(s.feat), lengths=s.history[..., 2].astype(np.uint32), cam=s.cam, px_dim=s.px)


def sequence(pbr, dev, temporal, between=None):
    """Two calls with a camera move, pbr_update_vertices, a third call -> the three steps, the vertices of the last two and
    facesV.  between( step 2 ): called before the vertices are updated."""
    sc, px, cams = hand_scene(pbr, dev)
    dev.temporal_track_motion(True)
    s1 = public_step(pbr, dev, px, cams[0], 0, temporal)
    s2 = public_step(pbr, dev, px, cams[1], 100, temporal)
    if between is not None:
        between(s2)
    before = dev.read_geometry()[0]
    target = hand_scenes.moved(sc)[0].copy()
    target.reshape(-1, 3, 4)[::2] = before.reshape(-1, 3, 4)[::2]                    # three vertices per face: every second face stays
    dev.update_vertices(target)
    after = dev.read_geometry()[0]
    s3 = public_step(pbr, dev, px, cams[1], 200, temporal, motion=True)
    return (s1, s2, s3), before, after, sc.arrays["facesV"]


@pytest.mark.parametrize("tparams", [{}, dict(max_history=2, normal_cos=0.99, sigma_world=0.0)], ids=["defaults", "short-strict"])
def test_pbr_denoise_temporal_is_the_diag_entry_on_its_own_planes(pbr, device, tparams):
    temporal = pbr.TemporalParams(**tparams)
    (s1, s2, s3), before, after, faces_v = sequence(pbr, device, temporal)
    assert not same_values(before, after)
    first = device.diag_temporal(s1.image, s1.var, np.stack(s1.feat), s1.cam, s1.px, temporal)
    assert same_values(first["integrated"], s1.integrated) and same_values(first["history"], s1.history) and (first["lengths"] == 1).all()
    second = device.diag_temporal(s2.image, s2.var, np.stack(s2.feat), s2.cam, s2.px, temporal, prev=as_previous(s1))
    assert same_values(second["integrated"], s2.integrated), describe_mismatch(second["integrated"], s2.integrated)
    assert same_values(second["history"], s2.history), describe_mismatch(second["history"], s2.history)
    third = device.diag_temporal(s3.image, s3.var, np.stack(s3.feat), s3.cam, s3.px, temporal, prev=as_previous(s2),
                                 motion=dict(face=s3.face, faces_v=faces_v, vertices=after, hist_vertices=before))
    assert same_values(third["motion"], s3.motion), describe_mismatch(third["motion"], s3.motion)
    assert same_values(third["integrated"], s3.integrated), describe_mismatch(third["integrated"], s3.integrated)
    assert same_values(third["history"], s3.history), describe_mismatch(third["history"], s3.history)
    assert same_values(third["lengths"], s3.history[..., 2])
    # the sequence did what it is there for: a history that is reused, hits and misses, moved and unmoved faces
    hit = s3.feat[1][..., 3] != 0
    assert ((s3.face >= 0) == hit).all() and 0.1 < hit.mean() < 1.0
    assert (s2.history[..., 2] >= 2).sum() > 20 and (s3.history[..., 2] >= 2).sum() > 0
    assert (s3.motion[..., 3] == 2).sum() > 10 and (s3.motion[..., 3] == 1).sum() > 10
    print("%r: call 2 L >= 2 on %d pixels, call 3 on %d; motion codes %r" % (tparams, (s2.history[..., 2] >= 2).sum(), (s3.history[..., 2] >= 2).sum(),
          dict(zip(*np.unique(s3.motion[..., 3], return_counts=True)))))


# ---- c: the entry leaves the context alone, and refuses what it says it refuses -----------------------------------------------

def test_the_diag_entry_leaves_the_context_alone(pbr, device):
    temporal = pbr.TemporalParams()
    plain, _, _, _ = sequence(pbr, device, temporal)
    seen = {}

    def between(s2):
        seen["ms"], seen["counters"], seen["image"] = device.last_kernel_ms(), device.counters(), device.read_output()
        for name in ("size_65x5_motion", "shift_hxy", "max_history_2_hxy", "first_call", "motion_all_faces"):
            case = next(c for c in T.cases() if c.name == name)
            got = device.diag_temporal(**T.device_inputs(pbr, case))
            assert same_values(got["integrated"], T.evaluate(case).rest.integrated)
        assert device.last_kernel_ms() == seen["ms"] and device.counters() == seen["counters"]
        assert same_values(device.read_output(), seen["image"])

    device.temporal_reset()
    mixed, _, _, _ = sequence(pbr, device, temporal, between)
    assert seen
    for a, b in zip(plain, mixed):
        for key in ("rgba", "var_out", "integrated", "history"):
            assert same_values(getattr(a, key), getattr(b, key)), key
    assert same_values(plain[2].motion, mixed[2].motion) and same_values(plain[2].face, mixed[2].face)
    assert (mixed[1].history[..., 2] >= 2).sum() > 20


def test_a_refused_call_is_einval_and_writes_nothing(pbr, planes_device):
    case = next(c for c in T.cases() if c.name == "motion_all_faces")
    good = T.device_inputs(pbr, case)
    h, w = case.h, case.w

    def refused(**changes):
        args = dict(good)
        for key, value in changes.items():
            if key in ("prev", "motion") and isinstance(value, dict):
                args[key] = dict(good[key], **value)
            else:
                args[key] = value
        out = {k: np.full((h, w, 4), 7.0, F) for k in ("integrated", "history", "motion", "reference")}
        out["lengths"] = np.full((h, w), 7, np.uint32)
        if args["motion"] is None:
            out.pop("motion"), out.pop("reference")
        with pytest.raises(pbr.PbrError, match=PBR_EINVAL):
            planes_device.diag_temporal(out=out, **args)
        assert all((a == 7).all() for a in out.values()), changes

    planes_device.diag_temporal(**good)                                           # the unchanged arguments are fine
    refused(motion=None, prev=None, temporal=pbr.TemporalParams(max_history=0))
    refused(temporal=pbr.TemporalParams(max_history=1025))
    refused(temporal=pbr.TemporalParams(normal_cos=1.5))
    refused(temporal=pbr.TemporalParams(normal_cos=float("nan")))
    refused(temporal=pbr.TemporalParams(sigma_world=-1.0))
    refused(temporal=pbr.TemporalParams(sigma_world=float("inf")))
    refused(prev=None)                                                            # motion inputs without a previous state
    face = case.motion.face.copy()
    face[2, 3] = len(case.motion.faces_v)
    refused(motion=dict(face=face))
    face[2, 3] = -2
    refused(motion=dict(face=face))
    faces_v = case.motion.faces_v.copy()
    faces_v[5, 1] = len(case.motion.vertices)
    refused(motion=dict(faces_v=faces_v))
    faces_v[5, 1] = 0xFFFFFFFF
    refused(motion=dict(faces_v=faces_v))
    for bad in (0, 1025, 0xFFFFFFFF):
        lengths = case.prev.lengths.astype(np.uint32)
        lengths[4, 6] = bad
        refused(prev=dict(lengths=lengths))
        refused(motion=None, prev=dict(lengths=lengths))
    # null and size errors, below the wrapper
    hip, ctx, cam, p = pbr.hip, planes_device._ctx, good["cam"], good["temporal"]
    image, var, feat = (np.ascontiguousarray(good[k], F) for k in ("image", "variance", "features"))
    out, lengths = np.full((h, w, 4), 7.0, F), np.full((h, w), 7, np.uint32)
    fp, up = pbr._as_fp, lambda a: a.ctypes.data_as(pbr._up)
    tail = (None, None, None, None, 0.0, None, None, 0, None, None, 0)
    for width, height, c, t, i, v, f, o in ((0, h, cam, p, image, var, feat, out), (w, -1, cam, p, image, var, feat, out), (1 << 11, 1 << 10, cam, p, image, var, feat, out),
                                            (w, h, None, p, image, var, feat, out), (w, h, cam, None, image, var, feat, out), (w, h, cam, p, None, var, feat, out),
                                            (w, h, cam, p, image, None, feat, out), (w, h, cam, p, image, var, None, out), (w, h, cam, p, image, var, feat, None)):
        status = hip.pbr_diag_temporal(ctx, width, height, float(case.px_dim), c, t, None if i is None else fp(i), None if v is None else fp(v),
                                       None if f is None else fp(f), *tail, None if o is None else fp(o), fp(out), up(lengths), None, None)
        assert status == -1 and (out == 7).all() and (lengths == 7).all()
    # a previous state given in part
    status = hip.pbr_diag_temporal(ctx, w, h, float(case.px_dim), cam, p, fp(image), fp(var), fp(feat), fp(image), None, None, None, 0.0,
                                   None, None, 0, None, None, 0, fp(out), fp(out), up(lengths), None, None)
    assert status == -1 and (out == 7).all() and (lengths == 7).all()


# ---- d: which decisions do the Cornell sequences take? --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_count_the_decisions_of_the_cornell_sequences(pbr, device, name):
    """Printed, not asserted (but for the device's agreement with the record's restatement): the pixels and taps per decision,
    over the calls of the sequence that have a history."""
    brdf, w, h, tparams, views = SEQUENCES[name]
    sc, cfg, px = cornell(pbr, device, brdf, w, h)
    temporal = pbr.TemporalParams(**tparams)
    total, prev = collections.Counter(), None
    for k, move in enumerate(views):
        s = cornell_step(pbr, device, px, view(pbr, sc, **move), 100 * k, temporal)
        if prev is not None:
            record = ref.Record(h, w)
            _, history = ref.integrate(s.image, s.var, s.feat, s.cam, s.px, ref.previous(prev.integrated, prev.feat, prev.history[..., 2], prev.cam, prev.px),
                                       temporal, record=record)
            assert same_values(history, s.history)
            case = types.SimpleNamespace(w=w, h=h, params=temporal)
            total.update(cpu.decision_counts(case, record, history))             # update, not +=: a count of 0 stays in the table
            total["C or V not finite (pixels)"] += int((~np.isfinite(np.concatenate([s.image[..., :3], s.var[..., None]], -1)).all(-1)).sum())
            total["I' not finite (pixels)"] += int((~np.isfinite(prev.integrated).all(-1)).sum())
            total["prev L == max_history - 1"] += int((prev.history[..., 2] == temporal.max_history - 1).sum())
            total["miss pixels"] += int((s.feat[1][..., 3] == 0).sum())
        prev = s
    COUNTED[name] = total
    print("\n%s (%d x %d, %d calls with a history):" % (name, w, h, len(views) - 1))
    for key in sorted(total):
        print("  %-36s %8d" % (key, total[key]))


def test_count_the_decisions_of_all_cornell_sequences():
    """The sum of the counts above (of those that ran), and the decisions no sequence takes at all."""
    total = collections.Counter()
    for counts in COUNTED.values():
        total.update(counts)
    print("\nall of %s:" % ", ".join(sorted(COUNTED)))
    for key in sorted(total):
        print("  %-36s %8d" % (key, total[key]))
    print("never taken: %s" % "; ".join(key for key in sorted(total) if total[key] == 0))
