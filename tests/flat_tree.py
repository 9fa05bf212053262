"""check_flat_tree: what every tree in the reference's flat format has to satisfy, whoever built it (numpy only)."""
import numpy as np

CAPS = (4000, 2000)


def check_flat_tree(nodes, facesV_out, facesV_in, vertices, sample=CAPS):
    """Structural invariants of the reference's flat format for a tree with <= 2 faces per leaf.  The boxes of the first
    sample[0] leaves and sample[1] containers are recomputed (large trees, for speed); sample=None: of every node."""
    n = nodes.shape[0]
    leaf = nodes[:, 3] >= 0
    assert not leaf[0] and nodes[0, 3] == -1
    # every face exactly once, in leaf order
    first = nodes[leaf, 3].astype(np.int64)
    second = nodes[leaf, 7].astype(np.int64)
    assert ((second == -1) | (second == first + 1)).all()
    covered = np.sort(np.concatenate([first, second[second >= 0]]))
    assert np.array_equal(covered, np.arange(facesV_in.shape[0]))
    key = lambda f: np.sort(f.view([("", f.dtype)] * 4).ravel())
    assert np.array_equal(key(np.ascontiguousarray(facesV_out)), key(np.ascontiguousarray(facesV_in)))      # a permutation of the input
    # depth-first order: a container's subtree is [i + 1, end) with end = its miss link, or the enclosing end
    end = np.empty(n, np.int64)
    stack = [n]
    for i in range(n):
        while stack and i >= stack[-1]:
            stack.pop()
        enclosing = stack[-1] if stack else n
        if leaf[i]:
            end[i] = i + 1
        else:
            link = int(nodes[i, 7])
            assert link == -1 or i + 1 < link <= n
            end[i] = link if link != -1 else enclosing
            assert end[i] <= enclosing
            stack.append(end[i])
    # boxes: a leaf's box is the exact bound of its faces, a container's the bound of its subtree's leaves
    leaves_cap, containers_cap = (None, None) if sample is None else sample
    tri = vertices[facesV_out[:, :3].astype(np.int64), :3]                    # (m, 3, 3)
    flo, fhi = tri.min(1), tri.max(1)
    for i in np.nonzero(leaf)[0][:leaves_cap]:
        f0, f1 = int(nodes[i, 3]), int(nodes[i, 7])
        lo, hi = flo[f0], fhi[f0]
        if f1 >= 0:
            lo, hi = np.minimum(lo, flo[f1]), np.maximum(hi, fhi[f1])
        assert np.array_equal(nodes[i, 0:3], lo) and np.array_equal(nodes[i, 4:7], hi)
    for i in np.nonzero(~leaf)[0][0:containers_cap]:
        sub = np.arange(i + 1, end[i])
        sub = sub[leaf[sub]]
        assert np.array_equal(nodes[i, 0:3], nodes[sub, 0:3].min(0)) and np.array_equal(nodes[i, 4:7], nodes[sub, 4:7].max(0))
