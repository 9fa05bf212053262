"""The tree pbr_build_bvh builds (csrc/bvh_build.hpp), restated in numpy binary32 operation by operation — the only definition
the build tests trust.  Finite vertices, at most 2^24 faces; every product, sum and quotient below is rounded to binary32.

  keys       per face: box = min / max of its three corners per component; centroid c = 0.5f * (min + max).
             Scene bounds lo / hi = min / max of the centroids under the order-preserving map of a float's bits to
             unsigned (sign set: ~bits, else bits | 0x80000000), so -0.0 is below +0.0.
             extent = hi - lo;  u = (c - lo) / extent where extent > 0, else 0;  q = uint( min( max( u * 8192, 0 ), 8191 ) )
             code = spread(qx) << 2 | spread(qy) << 1 | spread(qz), spread = bit b of 13 to bit 3 b;  key = code << 24 | face
  order      the keys are unique: ascending key order is THE order ("sorted position" below)

  ploc       ids [0, m) = the faces in sorted position, box = the face's; ids from m on = merges in creation order.
             Round over `count` clusters (positions 0 .. count - 1, radius r = radius_used):
               nearest  for position i, over pos = i + d, d = -r .. r, d != 0, 0 <= pos < count:
                        union box = min / max of the two boxes; half area = (x * y + z * y) + x * z of its extents hi - lo
                        the partner is the candidate least in (half area, pairKey( min(i, pos), max(i, pos) ),
                        min(i, pos), max(i, pos)) — pairKey in uint32 wraparound arithmetic
               flags    mutual: nearest[nearest[i]] == i; the lower position of a mutual pair merges, the upper is absorbed
               scan     slot = survivors before i, merge number = merges before i
               merge    id = nextNode + merge number: box = union; first child = the position's own cluster a, second = the
                        partner's b, exchanged when halfarea(b) > halfarea(a) (strict); two faces make a 2-face leaf of
                        size 1, anything else a container of size 1 + size(a) + size(b); faces add up; survivors keep
                        their order
             until one cluster is left (a round without a merge cannot happen with comparable boxes: ValueError)
             flatten  every id but a face inside a 2-face leaf: walking up, index += 1 + (second child ? size(first
                      sibling) : 0), firstFace += (second child ? faces(first sibling) : 0); record at `index`: a face or
                      2-face leaf = {box, firstFace, firstFace + 1 or -1} and its faces go to facesV/N_out[firstFace + k];
                      a container = {box, -1, index + size if < total else -1}

  lbvh       leaf l holds sorted positions 2 l and 2 l + 1 (the last may hold one); internal nodes [0, leaves - 1), then
             the leaves.  radixTree: Karras 2012 figure 4 over the FIRST key of each leaf, delta = count of leading zero
             bits of a ^ b, -1 outside the array.  Boxes bottom-up; a node's children are exchanged when
             halfarea(second) > halfarea(first); size = 1 + sizes.  flatten: index as above; a leaf = {box, 2 l, 2 l + 1
             or -1 past the last face}; faces stay in sorted position.

  wire       a tree that is one record gets a root in front of it: the same box, .w = -1 / -1 (2 nodes)
  radius     3 when the context is configured with an ordered traversal, else 32; a knob >= 1 replaces it; then [1, 64]

  held       what the cases of tests/bvh_build_cases.py decide trees by: the rounding order of the half area (skew), the
             pairKey tier of ties (strip, grid, repeated), the strict > of the exchange, the sign map's order of negative
             floats (wide).  NOT held by any case: the last tier of the tie order, (min, max) position after equal
             pairKeys — two pairs of one window with the same 32-bit pairKey do not occur at these sizes, so reversing it
             changes no tree here; and which zero a bound of -0.0 and +0.0 comes out as, which no tree depends on by value.

ploc / lbvh are vectorised over the device's threads; ploc_slow / lbvh_slow run one Python loop iteration per device thread
and share nothing with them but pair_key's constants: each checks the other (tests/test_bvh_build_ref_cpu.py).
"""
import numpy as np

MAX_RADIUS = 64
F32 = np.float32
_M32 = 0xFFFFFFFF


def radius_used(knob, traversal_configured):
    radius = 3 if traversal_configured else 32
    if knob >= 1:
        radius = knob
    return min(max(radius, 1), MAX_RADIUS)


def pair_key(lo, hi):
    """pairKey of bvh_build.hpp for Python ints."""
    h = (lo * 0x9E3779B1 + hi * 0x85EBCA77) & _M32
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & _M32
    h ^= h >> 12
    return h


def _pair_key_array(lo, hi):
    lo, hi = lo.astype(np.uint32), hi.astype(np.uint32)
    h = lo * np.uint32(0x9E3779B1) + hi * np.uint32(0x85EBCA77)          # uint32 arrays wrap
    h = h ^ (h >> np.uint32(15))
    h = h * np.uint32(0x2C1B3C6D)
    return h ^ (h >> np.uint32(12))


def expand_bits13(v):
    """expandBits13: bit b of the low 13 bits of v at bit 3 b."""
    x = np.asarray(v).astype(np.uint64) & np.uint64(0x1FFF)
    for shift, mask in ((32, 0x001F00000000FFFF), (16, 0x001F0000FF0000FF), (8, 0x100F00F00F00F00F),
                        (4, 0x10C30C30C30C30C3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(shift))) & np.uint64(mask)
    return x


def morton_code(q):
    """(…, 3) cell numbers -> 39-bit codes, x in the highest bit of each triple."""
    q = np.asarray(q)
    return (expand_bits13(q[..., 0]) << np.uint64(2)) | (expand_bits13(q[..., 1]) << np.uint64(1)) | expand_bits13(q[..., 2])


def _ordered(x):
    bits = np.ascontiguousarray(x, F32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000))


def _from_ordered(bits):
    bits = np.asarray(bits, np.uint32)
    return np.where(bits & np.uint32(0x80000000), bits & np.uint32(0x7FFFFFFF), ~bits).astype(np.uint32).view(F32)


def face_boxes(vertices, facesV):
    v = np.asarray(vertices, F32)[:, :3]
    tri = v[np.asarray(facesV)[:, :3].astype(np.int64)]                  # (m, 3, 3)
    return tri.min(1), tri.max(1)


def cells(vertices, facesV):
    """(m, 3) uint32: the cell of each face's centroid in the 8192^3 grid over the centroids' bounds."""
    lo, hi = face_boxes(vertices, facesV)
    c = F32(0.5) * (lo + hi)
    s_lo, s_hi = _from_ordered(_ordered(c).min(0)), _from_ordered(_ordered(c).max(0))
    extent = s_hi - s_lo
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(extent > 0, (c - s_lo) / extent, F32(0))
    return np.minimum(np.maximum(u * F32(8192), F32(0)), F32(8191)).astype(np.uint32)


def morton_keys(vertices, facesV):
    m = np.asarray(facesV).shape[0]
    return (morton_code(cells(vertices, facesV)) << np.uint64(24)) | np.arange(m, dtype=np.uint64)


def _half_area(lo, hi):
    e = hi - lo
    x, y, z = e[..., 0], e[..., 1], e[..., 2]
    return (x * y + z * y) + x * z


def _wire(records, facesV_out, facesN_out):
    if records.shape[0] == 1:
        root = records[0].copy()
        root[3] = root[7] = -1.0
        records = np.stack([root, records[0]])
    return records, facesV_out, facesN_out


def _inputs(vertices, facesV, facesN):
    vertices = np.ascontiguousarray(vertices, F32).reshape(-1, 4)
    facesV = np.ascontiguousarray(facesV, np.uint32).reshape(-1, 4)
    facesN = np.ascontiguousarray(facesN, np.uint32).reshape(-1, 4)
    keys = np.sort(morton_keys(vertices, facesV))
    return vertices, facesV, facesN, keys, (keys & np.uint64(0xFFFFFF)).astype(np.int64)


def _walk_up(ids, parent, left, right, size, faces):
    """index and firstFace of every id in `ids`: all the device's threads walk up together."""
    index, first = np.zeros(ids.shape[0], np.int64), np.zeros(ids.shape[0], np.int64)
    node, up = ids.copy(), parent[ids]
    while (up >= 0).any():
        live = up >= 0
        at = np.where(live, up, 0)
        second = live & (right[at] == node)
        index += live + np.where(second, size[left[at]], 0)
        if faces is not None:
            first += np.where(second, faces[left[at]], 0)
        node = np.where(live, up, node)
        up = np.where(live, parent[at], -1)
    return index, first


def ploc(vertices, facesV, facesN, radius, rounds=None):
    """rounds: a list that receives (boxes' lo, boxes' hi, merging positions (k, 2)) of every round, for tests."""
    vertices, facesV, facesN, _, order = _inputs(vertices, facesV, facesN)
    radius = min(max(int(radius), 1), MAX_RADIUS)
    m = facesV.shape[0]
    ids = 2 * m - 1
    left, right, parent = np.full(ids, -1, np.int64), np.full(ids, -1, np.int64), np.full(ids, -1, np.int64)
    size, faces = np.ones(ids, np.int64), np.ones(ids, np.int64)
    box_lo, box_hi = np.zeros((ids, 3), F32), np.zeros((ids, 3), F32)
    box_lo[:m], box_hi[:m] = face_boxes(vertices, facesV[order])
    clusters, next_node = np.arange(m, dtype=np.int64), m

    while clusters.shape[0] > 1:
        count = clusters.shape[0]
        reach = min(radius, count - 1)
        d = np.concatenate([np.arange(-reach, 0), np.arange(1, reach + 1)])
        i = np.arange(count)[:, None]
        pos = i + d[None, :]                                             # (count, 2 reach)
        valid = (pos >= 0) & (pos < count)
        at = np.clip(pos, 0, count - 1)
        lo, hi = box_lo[clusters], box_hi[clusters]
        area = _half_area(np.minimum(lo[:, None, :], lo[at]), np.maximum(hi[:, None, :], hi[at]))
        p_lo, p_hi = np.minimum(i, at), np.maximum(i, at)
        best = valid & (area == np.where(valid, area, np.inf).min(1)[:, None])
        key = _pair_key_array(p_lo, p_hi).astype(np.int64)
        best &= key == np.where(best, key, 1 << 32).min(1)[:, None]
        nearest = np.take_along_axis(at, np.where(best, p_lo * count + p_hi, count * count).argmin(1)[:, None], 1)[:, 0]

        here = np.arange(count)
        mutual = nearest[nearest] == here
        merges, absorbed = mutual & (here < nearest), mutual & (here > nearest)
        merged = int(merges.sum())
        if merged == 0:
            raise ValueError("clustering made no progress with %d clusters left" % count)
        if rounds is not None:
            rounds.append((lo, hi, np.stack([here[merges], nearest[merges]], 1)))
        new = next_node + np.cumsum(merges) - merges                     # exclusive scan
        a, b = clusters[merges], clusters[nearest[merges]]
        new_ids = new[merges]
        box_lo[new_ids], box_hi[new_ids] = np.minimum(box_lo[a], box_lo[b]), np.maximum(box_hi[a], box_hi[b])
        swap = _half_area(box_lo[b], box_hi[b]) > _half_area(box_lo[a], box_hi[a])
        left[new_ids], right[new_ids] = np.where(swap, b, a), np.where(swap, a, b)
        parent[a] = parent[b] = new_ids
        size[new_ids] = np.where((a < m) & (b < m), 1, 1 + size[a] + size[b])
        faces[new_ids] = faces[a] + faces[b]
        clusters = np.where(merges, new, clusters)[~absorbed]            # compaction keeps the order
        next_node += merged

    total = int(size[next_node - 1])
    emit = np.arange(next_node)
    is_face = emit < m
    up = np.where(parent[emit] >= 0, parent[emit], 0)
    inside = is_face & (parent[emit] >= 0) & (left[up] < m) & (right[up] < m)
    emit, is_face = emit[~inside], is_face[~inside]
    index, first = _walk_up(emit, parent, left, right, size, faces)
    leaf2 = ~is_face & (left[emit] < m) & (right[emit] < m)
    leaf = is_face | leaf2
    records = np.zeros((total, 8), F32)
    records[index, 0:3], records[index, 4:7] = box_lo[emit], box_hi[emit]
    nxt = index + size[emit]
    records[index, 3] = np.where(leaf, first, -1)
    records[index, 7] = np.where(leaf, np.where(leaf2, first + 1, -1), np.where(nxt < total, nxt, -1))
    outV, outN = np.zeros_like(facesV), np.zeros_like(facesN)
    member0 = np.where(is_face, emit, left[emit])[leaf]
    outV[first[leaf]], outN[first[leaf]] = facesV[order[member0]], facesN[order[member0]]
    member1 = right[emit][leaf2]
    outV[first[leaf2] + 1], outN[first[leaf2] + 1] = facesV[order[member1]], facesN[order[member1]]
    return _wire(records, outV, outN)


def _clz64(x):
    """Leading zero bits of non-zero uint64 values."""
    x = x.astype(np.uint64)
    n = np.zeros(x.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        empty = (x >> np.uint64(64 - s)) == 0
        n += np.where(empty, s, 0)
        x = np.where(empty, x << np.uint64(s), x)
    return n


def lbvh(vertices, facesV, facesN):
    vertices, facesV, facesN, keys, order = _inputs(vertices, facesV, facesN)
    m = facesV.shape[0]
    leaves = (m + 1) // 2
    internals, total = leaves - 1, 2 * leaves - 1
    first_key = keys[0::2]
    left, right, parent = np.full(total, -1, np.int64), np.full(total, -1, np.int64), np.full(total, -1, np.int64)

    if leaves > 1:
        i = np.arange(internals)

        def delta(j):
            inside = (j >= 0) & (j < leaves)
            return np.where(inside, _clz64(first_key[i] ^ first_key[np.where(inside, j, 0)]), -1)

        d = np.where(delta(i + 1) - delta(i - 1) >= 0, 1, -1)
        d_min = delta(i - d)
        l_max = np.full(internals, 2, np.int64)
        while True:
            grow = delta(i + l_max * d) > d_min
            if not grow.any():
                break
            l_max = np.where(grow, l_max * 2, l_max)
        l, t = np.zeros(internals, np.int64), l_max // 2
        while (t >= 1).any():
            l += np.where((t >= 1) & (delta(i + (l + t) * d) > d_min), t, 0)
            t //= 2
        j = i + l * d
        d_node = delta(j)
        s, t, live = np.zeros(internals, np.int64), (l + 1) // 2, np.ones(internals, bool)
        while live.any():
            s += np.where(live & (delta(i + (s + t) * d) > d_node), t, 0)
            live &= t != 1
            t = (t + 1) // 2
        split = i + s * d + np.where(d < 0, -1, 0)
        lo_end, hi_end = np.minimum(i, j), np.maximum(i, j)
        left[i] = np.where(split == lo_end, internals + split, split)
        right[i] = np.where(split + 1 == hi_end, internals + split + 1, split + 1)
        parent[left[i]] = i
        parent[right[i]] = i
        parent[0] = -1

    box_lo, box_hi = np.zeros((total, 3), F32), np.zeros((total, 3), F32)
    f_lo, f_hi = face_boxes(vertices, facesV[order])
    two = np.arange(leaves) * 2 + 1 < m
    other = np.where(two, np.arange(leaves) * 2 + 1, np.arange(leaves) * 2)
    box_lo[internals:], box_hi[internals:] = np.minimum(f_lo[0::2], f_lo[other]), np.maximum(f_hi[0::2], f_hi[other])
    size = np.ones(total, np.int64)
    done = np.arange(total) >= internals
    while not done.all():
        up = np.nonzero(~done[:internals] & done[left[:internals]] & done[right[:internals]])[0]
        a, b = left[up], right[up]
        box_lo[up], box_hi[up] = np.minimum(box_lo[a], box_lo[b]), np.maximum(box_hi[a], box_hi[b])
        size[up] = 1 + size[a] + size[b]
        swap = _half_area(box_lo[b], box_hi[b]) > _half_area(box_lo[a], box_hi[a])
        left[up], right[up] = np.where(swap, b, a), np.where(swap, a, b)
        done[up] = True

    emit = np.arange(total)
    index, _ = _walk_up(emit, parent, left, right, size, None)
    leaf = emit >= internals
    first = (emit - internals) * 2
    nxt = index + size
    records = np.zeros((total, 8), F32)
    records[index, 0:3], records[index, 4:7] = box_lo, box_hi
    records[index, 3] = np.where(leaf, first, -1)
    records[index, 7] = np.where(leaf, np.where(first + 1 < m, first + 1, -1), np.where(nxt < total, nxt, -1))
    return _wire(records, facesV[order], facesN[order])


# ----------------------------------------------------------------------------------------------------------------------
# The same, one Python loop iteration per device thread, in scalars.  Nothing above is called from here but pair_key.
# ----------------------------------------------------------------------------------------------------------------------
def _min(a, b):
    return a if a < b else b


def _max(a, b):
    return a if a > b else b


def _corner_box(vertices, face):
    a, b, c = (vertices[int(face[k])] for k in range(3))
    return ([_min(a[k], _min(b[k], c[k])) for k in range(3)], [_max(a[k], _max(b[k], c[k])) for k in range(3)])


def _ordered_slow(x):
    bits = int(np.array([x], F32).view(np.uint32)[0])
    return (~bits & _M32) if bits & 0x80000000 else (bits | 0x80000000)


def _from_ordered_slow(bits):
    bits = (bits & 0x7FFFFFFF) if bits & 0x80000000 else (~bits & _M32)
    return np.array([bits], np.uint32).view(F32)[0]


def _spread_slow(v):
    return sum(((v >> b) & 1) << (3 * b) for b in range(13))


def keys_slow(vertices, facesV):
    vertices, facesV = np.asarray(vertices, F32), np.asarray(facesV)
    m = facesV.shape[0]
    centroid = []
    for f in range(m):
        lo, hi = _corner_box(vertices, facesV[f])
        centroid.append([F32(0.5) * (lo[k] + hi[k]) for k in range(3)])
    s_min, s_max = [0xFF800000] * 3, [0x007FFFFF] * 3                     # images of +inf / -inf
    for f in range(m):
        for k in range(3):
            s_min[k] = min(s_min[k], _ordered_slow(centroid[f][k]))
            s_max[k] = max(s_max[k], _ordered_slow(centroid[f][k]))
    keys = []
    for f in range(m):
        q = []
        for k in range(3):
            lo, hi = _from_ordered_slow(s_min[k]), _from_ordered_slow(s_max[k])
            extent = hi - lo
            u = (centroid[f][k] - lo) / extent if extent > F32(0) else F32(0)
            q.append(int(_min(_max(u * F32(8192), F32(0)), F32(8191))))
        code = (_spread_slow(q[0]) << 2) | (_spread_slow(q[1]) << 1) | _spread_slow(q[2])
        keys.append((code << 24) | f)
    return keys


def _area_slow(lo, hi):
    x, y, z = hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]
    return (x * y + z * y) + x * z


def _before_slow(i, a, b):
    a_lo, a_hi = (a, i) if a < i else (i, a)
    b_lo, b_hi = (b, i) if b < i else (i, b)
    return a_lo < b_lo or (a_lo == b_lo and a_hi < b_hi)


def _wire_slow(records, outV, outN):
    if len(records) == 1:
        records = [records[0][0:3] + [-1.0] + records[0][4:7] + [-1.0], records[0]]
    return np.array(records, F32).reshape(-1, 8), np.array(outV, np.uint32).reshape(-1, 4), np.array(outN, np.uint32).reshape(-1, 4)


def ploc_slow(vertices, facesV, facesN, radius):
    vertices, facesV, facesN = np.asarray(vertices, F32), np.asarray(facesV, np.uint32), np.asarray(facesN, np.uint32)
    radius = min(max(int(radius), 1), MAX_RADIUS)
    m = facesV.shape[0]
    sorted_keys = sorted(keys_slow(vertices, facesV))
    ids = 2 * m - 1
    left, right, parent, size, faces = [-1] * ids, [-1] * ids, [-1] * ids, [1] * ids, [1] * ids
    box = [None] * ids
    for i in range(m):                                                    # plocInit
        box[i] = _corner_box(vertices, facesV[sorted_keys[i] & 0xFFFFFF])
    clusters, next_node = list(range(m)), m

    while len(clusters) > 1:
        count = len(clusters)
        nearest = [-1] * count
        for i in range(count):                                            # plocNearest
            lo, hi = box[clusters[i]]
            best, best_key, best_pos = None, 0, -1
            for d in range(-radius, radius + 1):
                pos = i + d
                if d == 0 or pos < 0 or pos >= count:
                    continue
                o_lo, o_hi = box[clusters[pos]]
                area = _area_slow([_min(lo[k], o_lo[k]) for k in range(3)], [_max(hi[k], o_hi[k]) for k in range(3)])
                key = pair_key(min(pos, i), max(pos, i))
                if best_pos < 0 or area < best or (area == best and (key < best_key or (key == best_key and _before_slow(i, pos, best_pos)))):
                    best, best_key, best_pos = area, key, pos
            nearest[i] = best_pos
        flags = []
        for i in range(count):                                            # plocFlags
            mutual = nearest[i] >= 0 and nearest[nearest[i]] == i
            flags.append((not (mutual and i > nearest[i]), mutual and i < nearest[i]))
        slots, merge_numbers, s, n = [], [], 0, 0
        for i in range(count):                                            # exclusive scan
            slots.append(s)
            merge_numbers.append(n)
            s, n = s + flags[i][0], n + flags[i][1]
        if n == 0:
            raise ValueError("clustering made no progress with %d clusters left" % count)
        following = [None] * s
        for i in range(count):                                            # plocMerge
            if not flags[i][0]:
                continue
            node = clusters[i]
            if flags[i][1]:
                other, merged = clusters[nearest[i]], next_node + merge_numbers[i]
                (a_lo, a_hi), (b_lo, b_hi) = box[node], box[other]
                box[merged] = ([_min(a_lo[k], b_lo[k]) for k in range(3)], [_max(a_hi[k], b_hi[k]) for k in range(3)])
                swap = _area_slow(b_lo, b_hi) > _area_slow(a_lo, a_hi)
                left[merged], right[merged] = (other, node) if swap else (node, other)
                parent[node] = parent[other] = merged
                size[merged] = 1 if node < m and other < m else 1 + size[node] + size[other]
                faces[merged] = faces[node] + faces[other]
                node = merged
            following[slots[i]] = node
        clusters, next_node = following, next_node + n

    total = size[next_node - 1]
    records, outV, outN = [None] * total, [None] * m, [None] * m
    for node in range(next_node):                                         # plocFlatten
        is_face = node < m
        up = parent[node]
        if is_face and up >= 0 and left[up] < m and right[up] < m:
            continue
        index, first, at = 0, 0, node
        while up >= 0:
            second = right[up] == at
            index += 1 + (size[left[up]] if second else 0)
            first += faces[left[up]] if second else 0
            at, up = up, parent[up]
        leaf2 = not is_face and left[node] < m and right[node] < m
        lo, hi = box[node]
        if is_face or leaf2:
            members = [node if is_face else left[node], right[node] if leaf2 else -1]
            for k in range(2):
                if members[k] >= 0:
                    face = sorted_keys[members[k]] & 0xFFFFFF
                    outV[first + k], outN[first + k] = facesV[face], facesN[face]
            words = (float(first), float(first + 1) if leaf2 else -1.0)
        else:
            nxt = index + size[node]
            words = (-1.0, float(nxt) if nxt < total else -1.0)
        records[index] = list(lo) + [words[0]] + list(hi) + [words[1]]
    return _wire_slow(records, outV, outN)


def lbvh_slow(vertices, facesV, facesN):
    vertices, facesV, facesN = np.asarray(vertices, F32), np.asarray(facesV, np.uint32), np.asarray(facesN, np.uint32)
    m = facesV.shape[0]
    sorted_keys = sorted(keys_slow(vertices, facesV))
    leaves = (m + 1) // 2
    internals, total = leaves - 1, 2 * leaves - 1
    left, right, parent, size = [-1] * total, [-1] * total, [-1] * total, [0] * total
    box = [None] * total

    def prefix(i, j):
        if j < 0 or j >= leaves:
            return -1
        return 64 - (sorted_keys[2 * i] ^ sorted_keys[2 * j]).bit_length()

    for i in range(internals):                                            # radixTree
        d = 1 if prefix(i, i + 1) - prefix(i, i - 1) >= 0 else -1
        d_min = prefix(i, i - d)
        l_max = 2
        while prefix(i, i + l_max * d) > d_min:
            l_max *= 2
        l, t = 0, l_max // 2
        while t >= 1:
            if prefix(i, i + (l + t) * d) > d_min:
                l += t
            t //= 2
        j = i + l * d
        d_node = prefix(i, j)
        s, t = 0, (l + 1) // 2
        while True:
            if prefix(i, i + (s + t) * d) > d_node:
                s += t
            if t == 1:
                break
            t = (t + 1) // 2
        split = i + s * d + (-1 if d < 0 else 0)
        lo_end, hi_end = min(i, j), max(i, j)
        left[i] = internals + split if split == lo_end else split
        right[i] = internals + split + 1 if split + 1 == hi_end else split + 1
        parent[left[i]] = parent[right[i]] = i

    outV, outN = [None] * m, [None] * m
    arrived = [0] * total
    for leaf in range(leaves):                                            # boxesBottomUp
        lo, hi = [F32(np.inf)] * 3, [F32(-np.inf)] * 3
        for k in range(2):
            at = 2 * leaf + k
            if at < m:
                face = sorted_keys[at] & 0xFFFFFF
                f_lo, f_hi = _corner_box(vertices, facesV[face])
                lo, hi = [_min(lo[c], f_lo[c]) for c in range(3)], [_max(hi[c], f_hi[c]) for c in range(3)]
                outV[at], outN[at] = facesV[face], facesN[face]
        node = internals + leaf
        box[node], size[node] = (lo, hi), 1
        up = parent[node]
        while up >= 0:
            arrived[up] += 1
            if arrived[up] == 1:
                break
            a, b = left[up], right[up]
            (a_lo, a_hi), (b_lo, b_hi) = box[a], box[b]
            box[up] = ([_min(a_lo[c], b_lo[c]) for c in range(3)], [_max(a_hi[c], b_hi[c]) for c in range(3)])
            size[up] = 1 + size[a] + size[b]
            if _area_slow(b_lo, b_hi) > _area_slow(a_lo, a_hi):
                left[up], right[up] = b, a
            node, up = up, parent[up]

    records = [None] * total
    for node in range(total):                                             # flatten
        index, at, up = 0, node, parent[node]
        while up >= 0:
            index += 1 + (size[left[up]] if right[up] == at else 0)
            at, up = up, parent[up]
        lo, hi = box[node]
        if node >= internals:
            first = (node - internals) * 2
            words = (float(first), float(first + 1) if first + 1 < m else -1.0)
        else:
            nxt = index + size[node]
            words = (-1.0, float(nxt) if nxt < total else -1.0)
        records[index] = list(lo) + [words[0]] + list(hi) + [words[1]]
    return _wire_slow(records, outV, outN)
