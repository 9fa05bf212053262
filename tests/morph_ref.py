"""pbr_set_morph / pbr_update_morph / pbr_update_pose (include/pbr_hip.h) restated in numpy binary32 — every array below is
float32 and every operation one numpy operation, so nothing is fused; no np.dot, no np.linalg — together with the element-major
transposition the library makes of the caller's lists and the targets and weight sets the tests give the fixtures.

  targets    a list with one (indices, deltas) pair per target: indices uint32, unique within the target; deltas (n, 3) float32
  active     the targets whose weight compares unequal to 0, in ascending target index
  position   p' = p; for every active target t that names the element, ascending: p'.c = p'.c + w_t * d.c; p'.w = p.w
  normal     q accumulated the same way; an element no active target names keeps n; else d = dot( q, q ), and
             !( d > 0 and d < inf ) keeps n too, otherwise n'.xyz = q * ( 1 / sqrt( d ) ), n'.w = n.w
  pose       skin_ref.skin of the morphed rest pose
"""
import zlib

import numpy as np

import transform_ref

F32 = np.float32
not_finite = transform_ref.not_finite


def _target(pair):
    index = np.asarray(pair[0], np.int64).reshape(-1)
    delta = np.asarray(pair[1], F32)
    delta = delta.reshape(index.shape[0], delta.shape[-1] if delta.ndim > 1 else 3)[:, :3]
    return index, delta


def accumulate(rest, targets, weights):
    """(q, touched): rest.xyz plus the active targets' weighted deltas, target after target, and which elements an active
    target names."""
    rest = np.asarray(rest, F32)
    weights = np.asarray(weights, F32).reshape(-1)
    assert len(targets) == weights.shape[0]
    q = rest[:, :3].copy()
    touched = np.zeros(rest.shape[0], bool)
    with np.errstate(all="ignore"):
        for t, pair in enumerate(targets):
            index, delta = _target(pair)
            if weights[t] == 0 or index.size == 0:
                continue
            assert np.unique(index).size == index.size
            q[index] = q[index] + weights[t] * delta
            touched[index] = True
    assert q.dtype == F32
    return q, touched


def positions(rest, targets, weights):
    """V': (vertices, 4) float32."""
    out = np.asarray(rest, F32).copy()
    out[:, :3] = accumulate(rest, targets, weights)[0]
    return out


def normals(rest_n, targets, weights):
    """N': (normals, 4) float32."""
    rest_n = np.asarray(rest_n, F32)
    q, touched = accumulate(rest_n, targets, weights)
    with np.errstate(all="ignore"):
        d = transform_ref._dot(q, q)
        unit = transform_ref._scale(q, F32(1.0) / np.sqrt(d))
    keep = ~touched | ~((d > 0) & (d < np.inf))
    out = rest_n.copy()
    out[:, :3] = np.where(keep[:, None], rest_n[:, :3], unit)
    assert out.dtype == F32
    return out


def morph(rest, vertex_targets, rest_n, normal_targets, weights):
    """(V', N') of one pbr_update_morph; N' is None without normal targets."""
    return positions(rest, vertex_targets, weights), (None if normal_targets is None else normals(rest_n, normal_targets, weights))


def lists(targets):
    """pbr_set_morph's target-major arguments: first (targets + 1) uint32, index uint32, delta (entries, 4) float32, w = 0."""
    pairs = [_target(p) for p in targets]
    first = np.zeros(len(pairs) + 1, np.uint32)
    first[1:] = np.cumsum([p[0].size for p in pairs])
    index = np.concatenate([p[0] for p in pairs] + [np.zeros(0, np.int64)]).astype(np.uint32)
    delta = np.zeros((index.size, 4), F32)
    delta[:, :3] = np.concatenate([p[1] for p in pairs] + [np.zeros((0, 3), F32)])
    return first, np.ascontiguousarray(index), np.ascontiguousarray(delta)


def pack(targets, count):
    """The element-major layout the kernels read: runFirst (count + 1) uint32, and per entry the delta (entries, 3) float32 and
    the target uint32 — an element's run in ascending target."""
    first, index, delta = lists(targets)
    target = np.repeat(np.arange(len(targets), dtype=np.uint32), np.diff(first.astype(np.int64)))
    order = np.argsort(index, kind="stable")                         # target-major input: stable keeps ascending target
    run_first = np.zeros(count + 1, np.uint32)
    run_first[1:] = np.cumsum(np.bincount(index, minlength=count))
    return run_first, np.ascontiguousarray(delta[order, :3]), np.ascontiguousarray(target[order])


def expected_bytes(num_vertices, vertex_targets, num_normals=0, normal_targets=None):
    """pbr_hip_diag.h: 16 V + 16 V + 4 ( V + 1 ) + 16 Ev, + 16 N + 4 ( N + 1 ) + 16 En with normal targets, + 4 T + 4."""
    ev = sum(_target(p)[0].size for p in vertex_targets)
    total = 32 * num_vertices + 4 * (num_vertices + 1) + 16 * ev + 4 * len(vertex_targets) + 4
    if normal_targets is not None:
        total += 16 * num_normals + 4 * (num_normals + 1) + 16 * sum(_target(p)[0].size for p in normal_targets)
    return total


# ---- the targets and weights of the fixtures ---------------------------------------------------------------------------------

BASE = 6          # targets 0 .. 5 follow the pattern below; Suzanne has more, all of them on one vertex
LONG = 296        # that vertex of Suzanne: a run of 66 — longer than a wave is wide — between neighbours with a run of 0
EXTRA = 66
KINDS = 8         # the pattern repeats every eight elements


def _members(count, dense):
    """Which elements each of the six base targets names.  With k = i % 8:
      k = 7, 0, 1  no target (a run of 0)          k = 2  target 2 alone
      k = 3        targets 0, 2, 3                 k = 4  every target that is not empty: 0, 2, 3, 4, 5
      k = 5        target 4 alone, a ZERO delta    k = 6  targets 3 and 5
    Target 1 is EMPTY.  dense: target 0 names EVERY element instead (no run of 0 is left then)."""
    k = np.arange(count) % KINDS
    every = np.ones(count, bool)
    return [every if dense else (k == 3) | (k == 4), np.zeros(count, bool), (k == 2) | (k == 3) | (k == 4), (k == 3) | (k == 4) | (k == 6),
            (k == 4) | (k == 5), (k == 4) | (k == 6)]


def targets_for(name, rest, rest_n, dense=False):
    """(vertex_targets, normal_targets) the tests give fixture `name`, seeded by the name.  Both follow _members over their own
    indices.  Vertex deltas are a few percent of the scene's extent, normal deltas about a third of a unit.  Target 4's deltas
    on elements with k = 5 are zero.  Normal target 2's delta on the normals with i % 16 == 2 is minus the rest normal: under
    weight 1.0 q is 0 and the rest normal is copied.  ref_suzanne_sa has EXTRA more targets that name vertex LONG alone (no
    normal)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    rest, rest_n = np.asarray(rest, F32), np.asarray(rest_n, F32)
    extent = float(np.abs(rest[:, :3]).max())
    out = []
    for array, size in ((rest, 0.04 * extent), (rest_n, 0.3)):
        count = array.shape[0]
        k = np.arange(count) % KINDS
        targets = []
        for t, member in enumerate(_members(count, dense)):
            index = np.flatnonzero(member)
            rng.shuffle(index)                                        # exporters do not sort
            delta = rng.uniform(-size, size, (index.size, 3)).astype(F32)
            if t == 4:
                delta[k[index] == 5] = 0.0
            if t == 2 and array is rest_n:
                cancel = index % 16 == 2
                delta[cancel] = -array[index[cancel], :3]
            targets.append((index.astype(np.uint32), delta))
        out.append(targets)
    if name == "ref_suzanne_sa":
        assert rest.shape[0] > LONG + 1
        for _ in range(EXTRA):
            out[0].append((np.array([LONG], np.uint32), rng.uniform(-0.01 * extent, 0.01 * extent, (1, 3)).astype(F32)))
            out[1].append((np.zeros(0, np.uint32), np.zeros((0, 3), F32)))
    return out[0], out[1]


def weights_for(num_targets):
    """The weight sets, by name: all 0; one-hot 1.0 on target 2; negatives; above 1; zeros between others; dyadic values.  Each
    repeats a short pattern over the targets."""
    t = np.arange(num_targets)
    one_hot = np.zeros(num_targets, F32)
    one_hot[2] = 1.0
    return {
        "all zero": np.zeros(num_targets, F32),
        "one-hot": one_hot,
        "negative": np.array([-0.3, -1.0, -0.55, -0.125, -0.8, -0.05], F32)[t % 6],
        "above one": np.array([1.5, 2.25, 1.1, 3.0, 1.75, 1.3], F32)[t % 6],
        "zeros between": np.array([0.7, 0.0, 0.4, 0.0, -0.6, 0.0, 1.2], F32)[t % 7],
        "dyadic": np.array([0.5, 0.25, -0.125, 1.0, 0.0625, 0.75], F32)[t % 6],
    }
