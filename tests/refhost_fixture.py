"""The recorded dumps of the reference's compiled host code (tests/golden/refhost_*.npz, tests/golden/make_refhost.py) as the
tests read them — numpy only, no reference, no dumper: the dumped tree by node id, the nodes PathTracer's flattening keeps,
and the flat arrays that flattening would upload, formed from the DUMP (never from this repository's builder).

PathTracer::initOpenCLBuffers_BVH (PathTracer.cpp:238-347) walks BVH::getNodes() — ids 0, 1, 2, ... in depth-first order, left
child first — and
  drops   the node after a container with skipNextLeft (its left child), and keeps dropping while the dropped node has the
          flag itself (:253-256, :271-273)
  writes  bbMin.w = index of the leaf's first face or -1, bbMax.w = of its second face or -1 (:267-268); for a container with
          a parent the miss link: a left child's is its right sibling's id - numSkipsToHere (:305); a right child's is that of
          the right sibling of the nearest ancestor that is a left child (:282-301), -1 when there is none
  appends each leaf's Tris: facesV[3 * face.w ..] with facesMtl[face.w] in .w, facesVN[3 * normals.w ..] with 0 (:312-330)
"""
import os

import numpy as np

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF
ID, DEPTH, SKIPS_TO_HERE, SKIP_NEXT_LEFT, PARENT, LEFT, RIGHT, FACES = range(8)       # columns of ref_tree_nodes

_cache = {}


PARTS = ("", "_tree", "_wire")      # a fixture too large for one file lies in three (tests/golden/make_refhost.py, save)


def files_of(name):
    return [p for p in (os.path.join(GOLDEN, name + part + ".npz") for part in PARTS) if os.path.exists(p)]


def load(name):
    """The fixture as a dict of arrays, its parts merged; loaded once, nobody writes to it."""
    if name not in _cache:
        data = {}
        for path in files_of(name):
            with np.load(path) as z:
                assert not set(z.files) & set(data)
                data.update({k: z[k] for k in z.files})
        for v in data.values():
            v.setflags(write=False)
        _cache[name] = data
    return _cache[name]


def alpha_of(d):
    settings = dict(zip(d["settings_keys"].tolist(), d["settings_values"].tolist()))
    return float(settings.get("render.phong_tessellation", 0.0))


class Flattened:
    """kept: ids of the nodes the flattening keeps, in order; bvh (n, 8) float32, facesV / facesN (m, 4) uint32: what it
    uploads; tri: for every uploaded face its row in ref_tri_* (the dump's leaf order); parent: for every kept node the
    position (in kept) of its nearest kept ancestor, -1 for the root."""


def flatten(d):
    t = d["ref_tree_nodes"].astype(np.int64)
    n = t.shape[0]
    assert np.array_equal(t[:, ID], np.arange(n)) and d["ref_nodes_in_id_order"][0, 0] == 1, "getNodes() is this depth-first order"
    boxes = d["ref_tree_boxes"]
    first_tri = np.concatenate([[0], np.cumsum(t[:, FACES])])               # the dump lists Tris in the same depth-first order
    fv, fvn, mtl = d["ref_facesV"], d["ref_facesVN"], d["ref_facesMtl"][:, 0]
    parent, left, right = t[:, PARENT], t[:, LEFT], t[:, RIGHT]
    root = lambda i: parent[i] == NONE

    def link_target(i):
        return int(t[i, ID] - t[i, SKIPS_TO_HERE])

    out = Flattened()
    kept, rows, faces_v, faces_n, tri_rows = [], [], [], [], []
    skip_next = False
    for i in range(n):
        if skip_next:
            skip_next = bool(t[i, SKIP_NEXT_LEFT])
            continue
        count = int(t[i, FACES])
        w_min = float(len(faces_v)) if count > 0 else -1.0
        w_max = float(len(faces_v) + 1) if count > 1 else -1.0
        if count == 0 and t[i, SKIP_NEXT_LEFT]:
            skip_next = True
        if not root(i) and count == 0:
            p = parent[i]
            if left[p] == i:
                w_max = link_target(right[p])
            elif not root(p):
                while right[parent[p]] == p:
                    p = parent[p]
                    if root(p):
                        break
                if not root(p):
                    w_max = link_target(right[parent[p]])
        kept.append(i)
        rows.append(np.concatenate([boxes[i, 0:3], [w_min], boxes[i, 3:6], [w_max]]))
        for k in range(first_tri[i], first_tri[i] + count):
            f, fn = int(d["ref_tri_face"][k, 3]), int(d["ref_tri_normals"][k, 3])
            faces_v.append([*fv[f], int(mtl[f]) & 0xFFFFFFFF])               # cl_int stored into cl_uint: -1 wraps
            faces_n.append([*fvn[fn], 0])
            tri_rows.append(k)
    out.kept = np.array(kept, np.int64)
    out.bvh = np.array(rows, np.float32)
    out.facesV, out.facesN = np.array(faces_v, np.uint32), np.array(faces_n, np.uint32)
    out.tri = np.array(tri_rows, np.int64)
    position = np.full(n, -1, np.int64)
    position[out.kept] = np.arange(out.kept.size)
    out.parent = np.full(out.kept.size, -1, np.int64)
    for k, i in enumerate(kept):
        p = parent[i]
        while p != NONE and position[p] < 0:
            p = parent[p]
        out.parent[k] = -1 if p == NONE else position[p]
    return out


def unflatten(bvh):
    """(leaf, end, parent) of a flat tree from its depth-first order, its leaf flags and its miss links alone: a container's
    subtree is [i + 1, end) with end = its miss link, or its enclosing subtree's end where the link is -1."""
    n = bvh.shape[0]
    leaf = bvh[:, 3] >= 0
    end, parent = np.empty(n, np.int64), np.full(n, -1, np.int64)
    stack = []                                                             # (node, end) of the open containers
    for i in range(n):
        while stack and i >= stack[-1][1]:
            stack.pop()
        parent[i] = stack[-1][0] if stack else -1
        enclosing = stack[-1][1] if stack else n
        if leaf[i]:
            end[i] = i + 1
        else:
            link = int(bvh[i, 7])
            end[i] = link if link != -1 else enclosing
            assert i + 1 < end[i] <= enclosing, "node %d: not nested" % i
            stack.append((i, end[i]))
    return leaf, end, parent
