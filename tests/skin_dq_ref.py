"""pbr_update_skin_dq / pbr_update_pose_dq (include/pbr_hip.h) restated in numpy binary32 — every array below is float32 and every
operation one numpy operation, so nothing is fused and `/` and sqrt are correctly rounded; no np.dot, no np.linalg — together with
the dual quaternions the tests give the bones, and an independent float64 reference that shares no algebra with rule 6.

  dot4        ( ( ax*bx + ay*by ) + az*bz ) + aw*bw
  slots       S = the slots j = 0..3 whose weight compares unequal to 0, in slot order
  hemisphere  pivot = the real part of the first slot of S; a later slot with dot4( r_s, pivot ) < 0 has its weight negated
  blend       first slot: Q[k] = w * q_s[k]; later ones: Q[k] = Q[k] + w * q_s[k]
  normalise   nn = dot4( Q.real, Q.real ), len = sqrt( nn ), r = Q.real / len, d = Q.dual / len
  identity    r.xyz == 0, |r.w| == 1, d == 0: the rest quad
  position    t = 2 cross( r.xyz, p ), u = cross( r.xyz, t ), p1 = ( p + r.w t ) + u, c = cross( r.xyz, d.xyz ),
              tr = 2 ( ( r.w d.xyz - d.w r.xyz ) + c ), p' = p1 + tr
  normal      q = ( n + r.w t ) + u from n, then transform_ref's tail; !( nn > 0 and nn < inf ) copies the rest normal
"""
import numpy as np

import morph_ref
import transform_ref
from patch_refit_ref import _cross, _dot, _scale

F32 = np.float32
SLOTS = 4
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0, 0], F32)


def _arrays(bones, weights):
    bones = np.asarray(bones, np.int64).reshape(-1, SLOTS)
    weights = np.asarray(weights, F32).reshape(-1, SLOTS)
    assert bones.shape == weights.shape
    return bones, weights


def _dot4(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]) + a[:, 3] * b[:, 3]


def hemisphere_dots(bones, weights, Q):
    """(elements, 4) float32: dot4( r_s, pivot ) of every slot behind the first active one, NaN for the others."""
    bones, weights = _arrays(bones, weights)
    Q = np.asarray(Q, F32).reshape(-1, 8)
    out = np.full(bones.shape, np.nan, F32)
    pivot = np.zeros((bones.shape[0], 4), F32)
    started = np.zeros(bones.shape[0], bool)
    for j in range(SLOTS):
        use = weights[:, j] != 0
        real = Q[bones[:, j], :4]
        first = use & ~started
        pivot = np.where(first[:, None], real, pivot)
        later = use & started
        out[later, j] = _dot4(real, pivot)[later]
        started = started | use
    return out


def blend(bones, weights, Q):
    """(r, d, nn): the normalised blend of every element, (elements, 4) twice, and the squared length it was divided by the root of."""
    bones, weights = _arrays(bones, weights)
    Q = np.asarray(Q, F32).reshape(-1, 8)
    S = np.zeros((bones.shape[0], 8), F32)
    pivot = np.zeros((bones.shape[0], 4), F32)
    started = np.zeros(bones.shape[0], bool)
    with np.errstate(all="ignore"):
        for j in range(SLOTS):
            w = weights[:, j]
            use = w != 0
            q = Q[bones[:, j]]
            first = use & ~started
            pivot = np.where(first[:, None], q[:, :4], pivot)
            w = np.where(~first & (_dot4(q[:, :4], pivot) < 0), -w, w)
            term = w[:, None] * q
            later = S + term
            S = np.where(use[:, None], np.where(started[:, None], later, term), S)
            started = started | use
        nn = _dot4(S[:, :4], S[:, :4])
        length = np.sqrt(nn)
        r = S[:, :4] / length[:, None]
        d = S[:, 4:] / length[:, None]
    assert r.dtype == d.dtype == nn.dtype == F32
    return r, d, nn


def is_identity(r, d):
    return (r[:, :3] == 0).all(axis=1) & (np.abs(r[:, 3]) == 1) & (d == 0).all(axis=1)


def _rotate(r, v):
    axis = r[:, :3]
    t = F32(2.0) * _cross(axis, v)
    u = _cross(axis, t)
    return (v + r[:, 3:4] * t) + u


def positions(rest, bones, weights, Q):
    """V': (vertices, 4) float32."""
    rest = np.asarray(rest, F32)
    r, d, _ = blend(bones, weights, Q)
    with np.errstate(all="ignore"):
        turned = _rotate(r, rest[:, :3])
        c = _cross(r[:, :3], d[:, :3])
        tr = F32(2.0) * ((r[:, 3:4] * d[:, :3] - d[:, 3:4] * r[:, :3]) + c)
        moved = turned + tr
    out = rest.copy()
    out[:, :3] = np.where(is_identity(r, d)[:, None], rest[:, :3], moved)
    assert out.dtype == F32
    return out


not_finite = transform_ref.not_finite


def normals(rest_n, bones, weights, Q):
    """N': (normals, 4) float32."""
    rest_n = np.asarray(rest_n, F32)
    r, d, nn = blend(bones, weights, Q)
    n = rest_n[:, :3]
    with np.errstate(all="ignore"):
        q = _rotate(r, n)
        dd = _dot(q, q)
        unit = _scale(q, F32(1.0) / np.sqrt(dd))
    keep = is_identity(r, d) | ~((nn > 0) & (nn < np.inf)) | ~((dd > 0) & (dd < np.inf))
    out = rest_n.copy()
    out[:, :3] = np.where(keep[:, None], n, unit)
    assert out.dtype == F32
    return out


def skin(rest, vertex_bones, vertex_weights, rest_n, normal_bones, normal_weights, Q):
    """(V', N') of one pbr_update_skin_dq; N' is None without normal influences."""
    return positions(rest, vertex_bones, vertex_weights, Q), (None if normal_bones is None else normals(rest_n, normal_bones, normal_weights, Q))


def pose(rest, vertex_targets, vertex_bones, vertex_weights, rest_n, normal_targets, normal_bones, normal_weights, morph_weights, Q):
    """(V', N') of one pbr_update_pose_dq: the morph (morph_ref), then the dq skin.  Normals: morphed with normal targets, skinned
    with normal influences, None with neither."""
    v = positions(morph_ref.positions(rest, vertex_targets, morph_weights), vertex_bones, vertex_weights, Q)
    n = None if normal_targets is None else morph_ref.normals(rest_n, normal_targets, morph_weights)
    if normal_bones is not None:
        n = normals(rest_n if n is None else n, normal_bones, normal_weights, Q)
    return v, n


def refused(Q, set_bones=None):
    """Why the two calls refuse these dual quaternions before they touch the device, in their order: ("count",), ("not finite",
    bone, word), ("zero real part", bone) or None."""
    Q = np.asarray(Q, F32).reshape(-1, 8)
    if set_bones is not None and Q.shape[0] != set_bones:
        return ("count",)
    bad = ~np.isfinite(Q)
    if bad.any():
        bone = int(np.argmax(bad.any(axis=1)))
        return "not finite", bone, int(np.argmax(bad[bone]))
    empty = (Q[:, :4] == 0).all(axis=1)
    return ("zero real part", int(np.argmax(empty))) if empty.any() else None


# ---- the bones of the tests --------------------------------------------------------------------------------------------------

def _qmul(a, b):
    """The quaternion product, ( x, y, z, w ) each, float64."""
    ax, ay, az, aw = np.moveaxis(np.asarray(a, np.float64), -1, 0)
    bx, by, bz, bw = np.moveaxis(np.asarray(b, np.float64), -1, 0)
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def dual_quat(axis, angle, translation, scale=1.0):
    """A turn by `angle` about `axis`, then a move by `translation`, in float64; the float32 cast is the bone.  `scale` multiplies
    all eight words: the same bone, not of unit length."""
    axis = np.asarray(axis, np.float64)
    axis = axis / np.sqrt((axis * axis).sum())
    r = np.concatenate([axis * np.sin(angle / 2.0), [np.cos(angle / 2.0)]])
    d = 0.5 * _qmul(np.concatenate([np.asarray(translation, np.float64), [0.0]]), r)
    return (scale * np.concatenate([r, d])).astype(F32)


_rng = np.random.default_rng(19)
BONE_NAMES = ("identity", "identity negated", "rotation about a skew axis", "turn of more than 180 degrees", "bone scaled by 3", "pure translation",
              "translation of 1e6", "seeded rotation a", "seeded rotation b")
BONES = np.stack([
    IDENTITY,
    -IDENTITY,
    dual_quat((1.0, 2.0, 3.0), 0.7, (0.25, -0.125, 0.0625)),
    dual_quat((0.0, 1.0, 0.5), np.radians(250.0), (-0.125, 0.25, 0.0)),            # cos( 125 degrees ) < 0: r.w < 0
    dual_quat((-1.0, 0.5, 2.0), 1.1, (0.1, -0.2, 0.3), scale=3.0),
    dual_quat((1.0, 0.0, 0.0), 0.0, (0.5, 0.0, -0.25)),
    dual_quat((1.0, 0.0, 0.0), 0.0, (1.0e6, -1.0e6, 1.0e6)),
    dual_quat(_rng.normal(size=3), _rng.uniform(0.2, 2.5), _rng.uniform(-0.3, 0.3, 3)),
    dual_quat(_rng.normal(size=3), _rng.uniform(0.2, 2.5), _rng.uniform(-0.3, 0.3, 3)),
])
assert BONES.dtype == F32 and BONES.shape == (len(BONE_NAMES), 8) and BONES[3, 3] < 0 and BONES[1, 3] == -1
# no pair of bones is exactly orthogonal in dot4: no hemisphere dot is 0, so negating a bone changes no bit
assert all(_dot4(BONES[a:a + 1, :4], BONES[b:b + 1, :4])[0] != 0 for a in range(len(BONES)) for b in range(len(BONES)))


def dual_quats_for(num_bones, shift=0, skip=()):
    """One bone of the set per bone of the skin, dealt round robin from `shift`; `skip` leaves names of the set out."""
    pool = [k for k, name in enumerate(BONE_NAMES) if name not in skip]
    return np.ascontiguousarray(BONES[[pool[(k + shift) % len(pool)] for k in range(num_bones)]])


# ---- the float64 reference ---------------------------------------------------------------------------------------------------

def reference(rest, bones, weights, Q):
    """(p', t, R) in float64 by another route: the blend with its hemisphere rule in double, the normalised dual quaternion as a
    3 x 3 rotation R and a translation t = 2 d r* (a full quaternion product), then p' = R p + t as a matrix product."""
    bones, weights = _arrays(bones, weights)
    Q = np.asarray(Q, F32).reshape(-1, 8).astype(np.float64)
    w = weights.astype(np.float64)
    count = bones.shape[0]
    S = np.zeros((count, 8))
    pivot = np.zeros((count, 4))
    started = np.zeros(count, bool)
    for j in range(SLOTS):
        use = w[:, j] != 0
        q = Q[bones[:, j]]
        first = use & ~started
        pivot[first] = q[first, :4]
        sign = np.where(started & ((q[:, :4] * pivot).sum(axis=1) < 0), -1.0, 1.0)
        S += np.where(use, sign * w[:, j], 0.0)[:, None] * q
        started |= use
    S /= np.sqrt((S[:, :4] ** 2).sum(axis=1))[:, None]
    x, y, z, s = S[:, 0], S[:, 1], S[:, 2], S[:, 3]
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)], axis=1),
                  np.stack([2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)], axis=1),
                  np.stack([2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)
    conj = S[:, :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    t = 2.0 * _qmul(S[:, 4:], conj)[:, :3]
    p = np.asarray(rest, np.float64)[:, :3]
    return np.einsum("nij,nj->ni", R, p) + t, t, R


def reference_normals(rest_n, bones, weights, Q):
    """R n to unit length, float64."""
    _, _, R = reference(np.zeros((np.asarray(rest_n).shape[0], 4)), bones, weights, Q)
    q = np.einsum("nij,nj->ni", R, np.asarray(rest_n, np.float64)[:, :3])
    return q / np.sqrt((q * q).sum(axis=1))[:, None]


def matrix_of(dual_quats):
    """Row-major 3 x 4 matrices, float64, of dual quaternions of any length: the round trip of pbr_dual_quats_from_matrices."""
    Q = np.asarray(dual_quats, np.float64).reshape(-1, 8)
    S = Q / np.sqrt((Q[:, :4] ** 2).sum(axis=1))[:, None]
    x, y, z, s = S[:, 0], S[:, 1], S[:, 2], S[:, 3]
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)], axis=1),
                  np.stack([2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)], axis=1),
                  np.stack([2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)
    t = 2.0 * _qmul(S[:, 4:], S[:, :4] * np.array([-1.0, -1.0, -1.0, 1.0]))[:, :3]
    return np.concatenate([R, t[:, :, None]], axis=2).reshape(-1, 12)
