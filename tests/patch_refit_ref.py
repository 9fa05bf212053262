"""The boxes pbr_update_geometry computes under Phong tessellation (include/pbr_hip.h), restated in numpy binary32 — every
array below is float32 and every operation one numpy operation, so nothing is fused and `/` and sqrt are correctly rounded —
and the seeded normals the tests move the patches with.  It reuses refit_ref's tree tables and container fold.

  face     lo = hi = corner a; fold b, c; with alpha > 0 and unequal normals fold the three raised corners and the nine edge
           points, in that order (a NaN point fails both compares and never enters)
  leaf     one running fold: its first face's points, then its second face's
  container, .w words   as refit_ref.refit
"""
import numpy as np

import refit_ref

F32 = np.float32
EDGE_UV = ((0.0, 0.5), (0.5, 0.0), (0.5, 0.5), (0.25, 0.75), (0.75, 0.25), (0.25, 0.0), (0.75, 0.0), (0.0, 0.25), (0.0, 0.75))


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _scale(a, s):
    """vector * scalar, per face: three multiplications."""
    return a * np.asarray(s, F32).reshape(-1, 1)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], axis=1)


def _on_plane(q, p, n):
    return q - _scale(n, _dot(q - p, n))


def phong_point(p, n, alpha, u, v):
    """p, n: three (faces, 3) float32 arrays each; u, v: (faces,) float32."""
    alpha = F32(alpha)
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    w = (F32(1.0) - u) - v
    bary = (_scale(p[0], u) + _scale(p[1], v)) + _scale(p[2], w)
    tess = (_scale(_on_plane(bary, p[0], n[0]), u) + _scale(_on_plane(bary, p[1], n[1]), v)) + _scale(_on_plane(bary, p[2], n[2]), w)
    return (F32(1.0) - alpha) * bary + alpha * tess


def face_points(p, n, alpha):
    """The points of every face in fold order, (faces, 3 or 15, 3) float32, and the mask of the faces whose extra twelve count
    (all points are computed for all faces; the mask says which enter)."""
    count = p[0].shape[0]
    if not alpha > 0.0:
        return np.stack(p, axis=1), np.zeros(count, bool)
    alpha = F32(alpha)
    with np.errstate(all="ignore"):
        t = (n[0] - n[1]) + (n[1] - n[2])
        curved = (np.abs(t) > F32(0.000001)).any(axis=1)
        e12, e13, e23, e31 = p[1] - p[0], p[2] - p[0], p[2] - p[1], p[0] - p[2]
        c12 = alpha * (_scale(n[1], _dot(n[1], e12)) - _scale(n[0], _dot(n[0], e12)))
        c23 = alpha * (_scale(n[2], _dot(n[2], e23)) - _scale(n[1], _dot(n[1], e23)))
        c31 = alpha * (_scale(n[0], _dot(n[0], e31)) - _scale(n[2], _dot(n[2], e31)))
        x = _cross(e12, e13)
        ng = _scale(x, F32(1.0) / np.sqrt(_dot(x, x)))
        m = _dot(ng, (c12 - c23) - c31)
        k = F32(1.0) / ((F32(4.0) * _dot(ng, c23)) * _dot(ng, c31) - m * m)
        u = k * ((F32(2.0) * _dot(ng, c23)) * _dot(ng, c31 + e31) + _dot(ng, c23 - e23) * m)
        v = k * ((F32(2.0) * _dot(ng, c31)) * _dot(ng, c23 - e23) + _dot(ng, c31 + e31) * m)
        u = np.where((u < 0) | (u > 1), F32(0.0), u)
        v = np.where((v < 0) | (v > 1), F32(0.0), v)
        apex = phong_point(p, n, alpha, u, v)
        thickness = _dot(ng, apex - p[0])
        raised = [p[c] + _scale(ng, thickness) for c in range(3)]
        edges = [phong_point(p, n, alpha, np.full(count, eu, F32), np.full(count, ev, F32)) for eu, ev in EDGE_UV]
    points = np.stack(list(p) + raised + edges, axis=1)
    assert points.dtype == F32
    return points, curved


def _gather(facesV, facesN, vertices, normals, faces):
    v, nn = np.asarray(vertices, F32)[:, :3], np.asarray(normals, F32)[:, :3]
    fv, fn = np.asarray(facesV)[faces][:, :3].astype(np.int64), np.asarray(facesN)[faces][:, :3].astype(np.int64)
    return [v[fv[:, k]] for k in range(3)], [nn[fn[:, k]] for k in range(3)]


def _fold_points(lo, hi, points, curved, where, first=0):
    """The running fold of `points` (faces, P, 3), from point `first` on, into lo / hi for the faces in `where`: the corners
    (points 0 .. 2) always, the rest if the face is curved."""
    for k in range(first, points.shape[1]):
        take = where & (curved | (k < 3))
        refit_ref._fold(lo, hi, points[:, k], points[:, k], take[:, None])


def face_boxes(facesV, facesN, vertices, normals, alpha):
    """(lo, hi), (faces, 3) float32 each: every face's box on its own."""
    faces = np.arange(np.asarray(facesV).shape[0])
    p, n = _gather(facesV, facesN, vertices, normals, faces)
    points, curved = face_points(p, n, alpha)
    lo, hi = points[:, 0].copy(), points[:, 0].copy()
    _fold_points(lo, hi, points, curved, np.ones(faces.size, bool), first=1)
    return lo, hi


def refit(bvh, facesV, facesN, vertices, normals, alpha):
    """The thick refit, (N, 8) float32: bvh's .w words, the boxes of the patches under alpha."""
    bvh = np.array(bvh, F32)
    leaf, face0, face1, end, parent = refit_ref.tree_tables(bvh)
    n = bvh.shape[0]
    lo, hi = np.zeros((n, 3), F32), np.zeros((n, 3), F32)

    leaves = np.nonzero(leaf)[0]
    p, nn = _gather(facesV, facesN, vertices, normals, face0[leaves])
    points, curved = face_points(p, nn, alpha)
    l_lo, l_hi = points[:, 0].copy(), points[:, 0].copy()
    _fold_points(l_lo, l_hi, points, curved, np.ones(leaves.size, bool), first=1)
    two = face1[leaves] >= 0
    p, nn = _gather(facesV, facesN, vertices, normals, np.where(two, face1[leaves], face0[leaves]))
    points, curved = face_points(p, nn, alpha)
    _fold_points(l_lo, l_hi, points, curved, two)
    lo[leaves], hi[leaves] = l_lo, l_hi

    h = refit_ref.heights(leaf, parent)
    for level in range(1, int(h.max()) + 1):            # children are lower than their parent
        nodes = np.nonzero(~leaf & (h == level))[0]
        c = nodes + 1
        a_lo, a_hi = lo[c].copy(), hi[c].copy()
        c = end[c]
        while (c < end[nodes]).any():
            more = c < end[nodes]
            at = np.where(more, c, nodes + 1)
            refit_ref._fold(a_lo, a_hi, lo[at], hi[at], more[:, None])
            c = np.where(more, end[at], c)
        lo[nodes], hi[nodes] = a_lo, a_hi

    bvh[:, 0:3], bvh[:, 4:7] = lo, hi
    return bvh


def pack_patches(facesV, facesN, vertices, normals):
    """packScene's triPN, (faces, 6, 4) float32: three corners, three normals, .w = 0."""
    faces = np.arange(np.asarray(facesV).shape[0])
    p, n = _gather(facesV, facesN, vertices, normals, faces)
    out = np.zeros((faces.size, 6, 4), F32)
    for k in range(3):
        out[:, k, :3], out[:, 3 + k, :3] = p[k], n[k]
    return out


def perturb_normals(normals, seed=1, amount=0.25):
    """Seeded new vertex normals: n + amount * sin( 5 n.yzx + phase ) with a seeded phase per axis, renormalised in float32.
    Finite; a function of the normal's value, so normals that were equal stay equal and a tree keeps its flat faces."""
    normals = np.asarray(normals, F32)
    phase = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, 3)
    moved = (normals[:, :3].astype(np.float64) + amount * np.sin(5.0 * normals[:, [1, 2, 0]].astype(np.float64) + phase)).astype(F32)
    length = np.sqrt((moved * moved).sum(axis=1, dtype=F32)).astype(F32)
    out = normals.copy()
    out[:, :3] = np.where(length[:, None] > 0, moved / np.where(length > 0, length, F32(1.0))[:, None], normals[:, :3]).astype(F32)
    assert np.isfinite(out).all() and out.dtype == F32
    return out
