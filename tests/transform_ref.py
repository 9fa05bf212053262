"""pbr_set_parts / pbr_update_transforms (include/pbr_hip.h) restated in numpy binary32 — every array below is float32 and every
operation one numpy operation, so nothing is fused and `/` and sqrt are correctly rounded; no np.dot, no np.linalg — together
with the parts the tests cut the fixtures into and the fixed matrix set they move them with.

  per part   c0 = cross( a1, a2 ), c1 = cross( a2, a0 ), c2 = cross( a0, a1 ), det = dot( a0, c0 ); det < 0 negates all nine
  position   p'.x = ( ( m0*p.x + m1*p.y ) + m2*p.z ) + m3, rows 1 and 2 likewise; .w stays
  normal     q.r = dot( c_r, n ), d = dot( q, q ); 0 < d < inf: q * ( 1 / sqrt( d ) ), else n; .w stays
  identity   a part whose twelve words equal the identity's as floats copies its rest words
"""
import numpy as np

from patch_refit_ref import _cross, _dot, _scale

F32 = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)


def _matrix(rows, translation):
    m = np.zeros((3, 4), np.float64)
    m[:, :3], m[:, 3] = rows, translation
    return m.astype(F32).reshape(12)


def _rotation(axis, angle):
    """Rodrigues' formula in float64, written out; the float32 cast is the matrix."""
    x, y, z = np.asarray(axis, np.float64) / np.sqrt(sum(v * v for v in axis))
    c, s = np.cos(angle), np.sin(angle)
    t = 1.0 - c
    return [[t * x * x + c, t * x * y - s * z, t * x * z + s * y],
            [t * x * y + s * z, t * y * y + c, t * y * z - s * x],
            [t * x * z - s * y, t * y * z + s * x, t * z * z + c]]


# the fixed matrix set, float32, in this order
MATRIX_NAMES = ("identity", "rotation about a skew axis", "non-uniform scale with translation", "mirror", "shear", "translation of 1e6")
MATRICES = np.stack([
    IDENTITY,
    _matrix(_rotation((1.0, 2.0, 3.0), 0.7), (0.25, -0.125, 0.0625)),
    _matrix(np.diag([1.5, 0.75, 1.25]), (0.1, -0.2, 0.3)),
    _matrix(np.diag([-1.0, 1.0, 1.0]), (0.5, 0.0, 0.0)),
    _matrix([[1.0, 0.3, 0.0], [0.0, 1.0, 0.2], [0.1, 0.0, 1.0]], (0.0, 0.0, 0.0)),
    _matrix(np.eye(3), (1.0e6, -1.0e6, 1.0e6)),
])
assert MATRICES.dtype == F32 and MATRICES.shape == (6, 12)


def matrices_for(num_parts, shift=0, skip=()):
    """One matrix of the set per part, dealt round robin from `shift`; `skip` leaves names of the set out."""
    pool = [k for k, name in enumerate(MATRIX_NAMES) if name not in skip]
    return np.ascontiguousarray(MATRICES[[pool[(k + shift) % len(pool)] for k in range(num_parts)]])


def is_identity(M):
    M = np.asarray(M, F32).reshape(-1, 12)
    return (M == IDENTITY).all(axis=1)


def cofactors(M):
    """(C, det): the nine words that travel with every part's twelve, (parts, 9) float32, and the determinants before the sign
    was taken out."""
    M = np.asarray(M, F32).reshape(-1, 12)
    a0, a1, a2 = M[:, 0:3], M[:, 4:7], M[:, 8:11]
    with np.errstate(all="ignore"):
        c0 = _cross(a1, a2)
        c1 = _cross(a2, a0)
        c2 = _cross(a0, a1)
        det = _dot(a0, c0)
    C = np.concatenate([c0, c1, c2], axis=1)
    C = np.where((det < 0)[:, None], -C, C)
    assert C.dtype == F32 and det.dtype == F32
    return C, det


def refused(M):
    """Why pbr_update_transforms refuses these matrices before it touches the device: (what, part) or None."""
    M = np.asarray(M, F32).reshape(-1, 12)
    bad = ~np.isfinite(M).all(axis=1)
    if bad.any():
        return "not finite", int(np.argmax(bad))
    C, det = cofactors(M)
    bad = ~np.isfinite(det) | (det == 0) | ~np.isfinite(C).all(axis=1)
    return ("determinant", int(np.argmax(bad))) if bad.any() else None


def positions(rest, part, M):
    """V': (vertices, 4) float32 from the rest positions, every vertex's part and the parts' matrices."""
    rest, M = np.asarray(rest, F32), np.asarray(M, F32).reshape(-1, 12)
    m = M[np.asarray(part, np.int64)]
    copy = is_identity(M)[np.asarray(part, np.int64)]
    out = rest.copy()
    with np.errstate(all="ignore"):
        for r in range(3):
            s = m[:, 4 * r] * rest[:, 0] + m[:, 4 * r + 1] * rest[:, 1]
            s = s + m[:, 4 * r + 2] * rest[:, 2]
            s = s + m[:, 4 * r + 3]
            out[:, r] = np.where(copy, rest[:, r], s)
    assert out.dtype == F32
    return out


def not_finite(vertices):
    """The vertices pbr_update_transforms' device check raises its flag for."""
    return ~np.isfinite(np.asarray(vertices, F32)[:, :3]).all(axis=1)


def normals(rest_n, part, C, identity):
    """N': (normals, 4) float32 from the rest normals, every normal's part, the parts' cofactor words and identity flags."""
    rest_n, C = np.asarray(rest_n, F32), np.asarray(C, F32).reshape(-1, 9)
    c = C[np.asarray(part, np.int64)]
    copy = np.asarray(identity, bool)[np.asarray(part, np.int64)]
    n = rest_n[:, :3]
    with np.errstate(all="ignore"):
        q = np.stack([_dot(c[:, 0:3], n), _dot(c[:, 3:6], n), _dot(c[:, 6:9], n)], axis=1)
        d = _dot(q, q)
        unit = _scale(q, F32(1.0) / np.sqrt(d))
    keep = copy | ~((d > 0) & (d < np.inf))
    out = rest_n.copy()
    out[:, :3] = np.where(keep[:, None], n, unit)
    assert out.dtype == F32
    return out


def transform(rest, vertex_part, rest_n, normal_part, M):
    """(V', N') of one pbr_update_transforms; N' is None without normal parts."""
    C, _ = cofactors(M)
    v = positions(rest, vertex_part, M)
    return v, (None if normal_part is None else normals(rest_n, normal_part, C, is_identity(M)))


# ---- the parts of the fixtures -----------------------------------------------------------------------------------------------

def _components(facesV, num_vertices):
    """Connected components of the vertices under shared faces, by union-find; ids in order of each component's first vertex."""
    parent = list(range(num_vertices))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for a, b, c in np.asarray(facesV)[:, :3].tolist():
        ra, rb, rc = find(a), find(b), find(c)
        low = min(ra, rb, rc)
        parent[ra] = parent[rb] = parent[rc] = low
    ids, part = {}, np.zeros(num_vertices, np.uint32)
    for i in range(num_vertices):
        part[i] = ids.setdefault(find(i), len(ids))
    return part, len(ids)


TEARING = 5     # the mesh-tearing split: vertex index % 5, declared with one part more than it uses


def parts_of(name, facesV, facesN, num_vertices, num_normals):
    """(vertex_part, normal_part, num_parts) the tests cut fixture `name` into: connected components — except ref_suzanne_sa, cut
    by vertex index % 5 so that faces span parts, with a sixth part id that stays empty.  A normal takes the part of the first
    vertex it is paired with in facesV / facesN (faces in order, corners in order); a normal no face uses is in part 0."""
    if name.startswith("ref_suzanne"):
        vertex_part, num_parts = (np.arange(num_vertices) % TEARING).astype(np.uint32), TEARING + 1
    else:
        vertex_part, num_parts = _components(facesV, num_vertices)
    normal_part = np.zeros(num_normals, np.uint32)
    if num_normals:
        pairs_n = np.asarray(facesN)[:, :3].reshape(-1).astype(np.int64)
        pairs_v = np.asarray(facesV)[:, :3].reshape(-1).astype(np.int64)
        used, first = np.unique(pairs_n, return_index=True)
        normal_part[used] = vertex_part[pairs_v[first]]
    return vertex_part, normal_part, num_parts
