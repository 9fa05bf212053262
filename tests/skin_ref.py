"""pbr_set_skin / pbr_update_skin (include/pbr_hip.h) restated in numpy binary32 — every array below is float32 and every
operation one numpy operation, so nothing is fused; no np.dot, no np.linalg — together with the influences the tests give the
fixtures.  Positions, cofactors and normals are transform_ref's, applied to one blended matrix per element.

  slots      S = the slots j = 0..3 whose weight compares unequal to 0, in slot order
  blend      first slot s of S: B[k] = w_s * m_s[k]; every later one: B[k] = B[k] + w_s * m_s[k]
  position   transform_ref.positions with B as the element's matrix, the identity rule included
  normal     transform_ref.cofactors( B ), then transform_ref.normals: a d that is 0, infinite or NaN copies the rest normal
"""
import numpy as np

import transform_ref

F32 = np.float32
SLOTS = 4


def _arrays(bones, weights):
    bones = np.asarray(bones, np.int64).reshape(-1, SLOTS)
    weights = np.asarray(weights, F32).reshape(-1, SLOTS)
    assert bones.shape == weights.shape
    return bones, weights


def blend(bones, weights, M):
    """B: (elements, 12) float32, the blended matrix of every element."""
    bones, weights = _arrays(bones, weights)
    M = np.asarray(M, F32).reshape(-1, 12)
    B = np.zeros((bones.shape[0], 12), F32)
    started = np.zeros(bones.shape[0], bool)
    with np.errstate(all="ignore"):
        for j in range(SLOTS):
            w = weights[:, j]
            use = w != 0
            term = w[:, None] * M[bones[:, j]]
            later = B + term
            B = np.where(use[:, None], np.where(started[:, None], later, term), B)
            started = started | use
    assert B.dtype == F32
    return B


def positions(rest, bones, weights, M):
    """V': (vertices, 4) float32 from the rest positions, every vertex's influences and the bones' matrices."""
    rest = np.asarray(rest, F32)
    return transform_ref.positions(rest, np.arange(rest.shape[0]), blend(bones, weights, M))


not_finite = transform_ref.not_finite


def normals(rest_n, bones, weights, M):
    """N': (normals, 4) float32 from the rest normals, every normal's influences and the bones' matrices."""
    rest_n = np.asarray(rest_n, F32)
    B = blend(bones, weights, M)
    C, _ = transform_ref.cofactors(B)
    return transform_ref.normals(rest_n, np.arange(rest_n.shape[0]), C, transform_ref.is_identity(B))


def skin(rest, vertex_bones, vertex_weights, rest_n, normal_bones, normal_weights, M):
    """(V', N') of one pbr_update_skin; N' is None without normal influences."""
    v = positions(rest, vertex_bones, vertex_weights, M)
    return v, (None if normal_bones is None else normals(rest_n, normal_bones, normal_weights, M))


def refused(M):
    """Why pbr_update_skin refuses these matrices before it touches the device: ("not finite", bone, word) or None.  A singular
    matrix is not refused."""
    M = np.asarray(M, F32).reshape(-1, 12)
    bad = ~np.isfinite(M)
    if bad.any():
        bone = int(np.argmax(bad.any(axis=1)))
        return "not finite", bone, int(np.argmax(bad[bone]))
    return None


def refused_influences(bones, weights, num_bones):
    """Why pbr_set_skin refuses one pair of arrays, in its order — all indices, then all weights, then the sums: (what, element,
    slot or None) or None."""
    bones, weights = _arrays(bones, weights)
    for what, bad in (("bone", bones >= num_bones), ("weight", ~np.isfinite(weights) | (weights < 0))):
        if bad.any():
            element = int(np.argmax(bad.any(axis=1)))
            return what, element, int(np.argmax(bad[element]))
    empty = (weights == 0).all(axis=1)
    return ("all zero", int(np.argmax(empty)), None) if empty.any() else None


# ---- the influences of the fixtures ------------------------------------------------------------------------------------------

KINDS = 8     # the pattern below repeats every eight vertices


def influences_for(name, facesV, facesN, num_vertices, num_normals):
    """(vertex_bones, vertex_weights, normal_bones, normal_weights, num_bones) the tests give fixture `name`.  The bones are the
    fixture's parts (transform_ref.parts_of) plus one bone that only slots of weight 0 name.  With p the vertex's own part and
    q, r, t the next three, cyclically, vertex i takes pattern i % 8:
      0  one-hot in slot 0                      1  one-hot, the 1.0 in slot 2
      2  two weights, 1/2 + 1/2                 3  three, 1/2 + 1/4 + 1/4
      4  four, .4 + .3 + .2 + .1                5  a zero weight between two others, 3/4 . 1/4
      6  the same bone in two slots             7  weights that sum to 1.3
    A normal takes the influences of the first vertex it is paired with in facesV / facesN; a normal no face uses, vertex 0's."""
    vertex_part, _, num_parts = transform_ref.parts_of(name, facesV, facesN, num_vertices, num_normals)
    unused, num_bones = num_parts, num_parts + 1
    p = vertex_part.astype(np.int64)
    q, r, t = (p + 1) % num_parts, (p + 2) % num_parts, (p + 3) % num_parts
    u = np.full_like(p, unused)
    kind = np.arange(num_vertices) % KINDS
    table = (
        ((p, u, q, u), (1.0, 0.0, 0.0, 0.0)),
        ((q, r, p, u), (0.0, 0.0, 1.0, 0.0)),
        ((p, q, u, u), (0.5, 0.5, 0.0, 0.0)),
        ((p, q, r, u), (0.5, 0.25, 0.25, 0.0)),
        ((p, q, r, t), (0.4, 0.3, 0.2, 0.1)),
        ((p, u, q, u), (0.75, 0.0, 0.25, 0.0)),
        ((p, p, q, u), (0.25, 0.25, 0.5, 0.0)),
        ((p, q, u, u), (0.7, 0.6, 0.0, 0.0)),
    )
    vertex_bones = np.zeros((num_vertices, SLOTS), np.uint32)
    vertex_weights = np.zeros((num_vertices, SLOTS), F32)
    for k, (bones, weights) in enumerate(table):
        rows = kind == k
        vertex_bones[rows] = np.stack(bones, axis=1)[rows]
        vertex_weights[rows] = np.array(weights, F32)
    source = np.zeros(num_normals, np.int64)
    if num_normals:
        pairs_n = np.asarray(facesN)[:, :3].reshape(-1).astype(np.int64)
        pairs_v = np.asarray(facesV)[:, :3].reshape(-1).astype(np.int64)
        used, first = np.unique(pairs_n, return_index=True)
        source[used] = pairs_v[first]
    return vertex_bones, vertex_weights, np.ascontiguousarray(vertex_bones[source]), np.ascontiguousarray(vertex_weights[source]), num_bones


def one_hot(part):
    """(bones, weights) of the skin that equals parts: every element's own part with weight 1.0 in slot 0, the other slots naming
    bone 0 with weight 0."""
    part = np.asarray(part, np.uint32)
    bones = np.zeros((part.shape[0], SLOTS), np.uint32)
    weights = np.zeros((part.shape[0], SLOTS), F32)
    bones[:, 0], weights[:, 0] = part, 1.0
    return bones, weights
