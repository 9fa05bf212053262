"""The boxes pbr_update_vertices computes (include/pbr_hip.h), restated in numpy binary32 — the only definition the refit
tests trust — and the seeded deformations they move the vertices with.

  leaf       per component: start from corner a of its first face; fold in b, c, then the second face's a, b, c if there is
             one, with lo = v if v < lo else lo and hi = v if v > hi else hi
  container  (node 0 included) the same fold over its children's boxes in depth-first child order, starting from the first
             child's box; the children of i are c0 = i + 1, c1 = end(c0), ... below end(i)
  .w words   unchanged
"""
import numpy as np


def tree_tables(bvh):
    """(leaf mask, first face, second face or -1, end, parent) of a flat tree in the wire format: a leaf ends at index + 1, a
    container at its miss link when that is > index, else where its parent ends (node 0: N)."""
    bvh = np.asarray(bvh, np.float32)
    n = bvh.shape[0]
    leaf = bvh[:, 3] != -1.0
    face0 = np.where(leaf, bvh[:, 3], -1).astype(np.int64)
    word = bvh[:, 7].astype(np.int64)
    end, parent, open_ = np.zeros(n, np.int64), np.full(n, -1, np.int64), []
    for i in range(n):
        while open_ and i >= end[open_[-1]]:
            open_.pop()
        parent[i] = open_[-1] if open_ else -1
        if leaf[i]:
            end[i] = i + 1
        else:
            end[i] = word[i] if word[i] > i else (end[open_[-1]] if open_ else n)
            open_.append(i)
    return leaf, face0, np.where(leaf, word, -1), end, parent


def children(i, end):
    c = i + 1
    while c < end[i]:
        yield c
        c = end[c]


def heights(leaf, parent):
    h = np.zeros(leaf.shape[0], np.int64)
    for i in range(leaf.shape[0] - 1, 0, -1):
        h[parent[i]] = max(h[parent[i]], h[i] + 1)
    return h


def _fold(lo, hi, v_lo, v_hi, where=True):
    lo[...] = np.where(where & (v_lo < lo), v_lo, lo)
    hi[...] = np.where(where & (v_hi > hi), v_hi, hi)


def refit(bvh, facesV, vertices):
    """The refitted nodes, (N, 8) float32: bvh's .w words, the boxes of `vertices`."""
    bvh = np.array(bvh, np.float32)
    facesV = np.asarray(facesV, np.uint32)
    v = np.asarray(vertices, np.float32)[:, :3]
    leaf, face0, face1, end, parent = tree_tables(bvh)
    n = bvh.shape[0]
    lo, hi = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)

    leaves = np.nonzero(leaf)[0]
    first = facesV[face0[leaves]]
    l_lo, l_hi = v[first[:, 0]].copy(), v[first[:, 0]].copy()
    for k in (1, 2):
        _fold(l_lo, l_hi, v[first[:, k]], v[first[:, k]])
    two = (face1[leaves] >= 0)[:, None]
    second = facesV[np.where(face1[leaves] >= 0, face1[leaves], face0[leaves])]
    for k in (0, 1, 2):
        _fold(l_lo, l_hi, v[second[:, k]], v[second[:, k]], two)
    lo[leaves], hi[leaves] = l_lo, l_hi

    h = heights(leaf, parent)
    for level in range(1, int(h.max()) + 1):            # children are lower than their parent
        nodes = np.nonzero(~leaf & (h == level))[0]
        c = nodes + 1
        a_lo, a_hi = lo[c].copy(), hi[c].copy()
        c = end[c]
        while (c < end[nodes]).any():
            more = c < end[nodes]
            at = np.where(more, c, nodes + 1)
            _fold(a_lo, a_hi, lo[at], hi[at], more[:, None])
            c = np.where(more, end[at], c)
        lo[nodes], hi[nodes] = a_lo, a_hi

    bvh[:, 0:3], bvh[:, 4:7] = lo, hi
    return bvh


def refit_slow(bvh, facesV, vertices):
    """The same, node by node as the header states it (small trees: checks the vectorised form above)."""
    bvh = np.array(bvh, np.float32)
    v = np.asarray(vertices, np.float32)[:, :3]
    leaf, face0, face1, end, _ = tree_tables(bvh)
    for i in range(bvh.shape[0] - 1, -1, -1):
        if leaf[i]:
            faces = [face0[i]] + ([face1[i]] if face1[i] >= 0 else [])
            boxes = [(v[int(facesV[f][k])], v[int(facesV[f][k])]) for f in faces for k in range(3)]
        else:
            boxes = [(bvh[c, 0:3], bvh[c, 4:7]) for c in children(i, end)]
        lo, hi = boxes[0][0].copy(), boxes[0][1].copy()
        for b_lo, b_hi in boxes[1:]:
            for k in range(3):
                lo[k] = b_lo[k] if b_lo[k] < lo[k] else lo[k]
                hi[k] = b_hi[k] if b_hi[k] > hi[k] else hi[k]
        bvh[i, 0:3], bvh[i, 4:7] = lo, hi
    return bvh


def scene_scales(facesV, vertices):
    """(median edge length, diagonal of the vertices' box)."""
    v = np.asarray(vertices, np.float64)[:, :3]
    f = np.asarray(facesV)[:, :3].astype(np.int64)
    edges = np.linalg.norm(v[f[:, 1]] - v[f[:, 0]], axis=1)
    return float(np.median(edges)), float(np.linalg.norm(v.max(0) - v.min(0)))


AMPLITUDES = ("small", "large")


def deform(facesV, vertices, amplitude, seed=1):
    """v + A sin( k v.yzx + seed ), finite and seeded.  "small": A = a quarter of the median edge, the triangles keep their
    neighbourhood; "large": A = a quarter of the scene's diagonal over three periods, sibling boxes overlap heavily."""
    vertices = np.asarray(vertices, np.float32)
    edge, diagonal = scene_scales(facesV, vertices)
    a = {"small": 0.25 * edge, "large": 0.25 * diagonal}[amplitude]
    k = 2.0 * np.pi * 3.0 / max(diagonal, 1e-6)
    v = vertices[:, :3].astype(np.float64)
    out = vertices.copy()
    out[:, :3] = (v + a * np.sin(k * v[:, [1, 2, 0]] + seed)).astype(np.float32)
    assert np.isfinite(out).all()
    return out
