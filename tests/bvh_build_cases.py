"""Seeded inputs for the device-build tests: (vertices (n, 4) float32, facesV (m, 4) uint32, facesN (m, 4) uint32) per family,
each the smallest that reaches the mechanism it is named for (numpy only).  facesN rows are distinct, so a facesN_out that
was permuted differently from facesV_out shows."""
import numpy as np


def _faces(corners, seed):
    """One triangle per row of corners (m, 3, 3): unshared vertices."""
    m = corners.shape[0]
    vertices = np.zeros((3 * m, 4), np.float32)
    vertices[:, :3] = corners.reshape(-1, 3)
    facesV = np.zeros((m, 4), np.uint32)
    facesV[:, :3] = np.arange(3 * m).reshape(m, 3)
    facesV[:, 3] = np.arange(m) % 5                                       # the material word travels with the face
    return vertices, facesV, normals_for(m, seed)


def normals_for(m, seed):
    facesN = np.random.default_rng(1000 + seed).integers(0, 1 << 20, (m, 4)).astype(np.uint32)
    facesN[:, 3] = np.arange(m)
    return facesN


def soup(m, seed=1, edge=0.05):
    """Random triangles in the unit cube."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0.0, 1.0, (m, 1, 3))
    return _faces(centre + rng.uniform(-0.5 * edge, 0.5 * edge, (m, 3, 3)), seed)


def permuted(m, seed=1):
    """soup( m, seed ) with its face list in another order: the same geometry under other face indices."""
    vertices, facesV, facesN = soup(m, seed)
    order = np.random.default_rng(50 + seed).permutation(m)
    return vertices, facesV[order], facesN[order]


def flat(m, seed=2):
    """The soup pressed onto z = 0, every third face onto z = -0.0: no extent on one axis.  The two zeros are there so that
    a build which tells them apart shows; they do not pin the ordered map of the bounds (c - -0.0 is c - +0.0, and the extent
    is the same either way): by value a -0.0 bound changes no tree."""
    vertices, facesV, facesN = soup(m, seed)
    vertices[:, 2] = 0.0
    vertices[0::9, 2] = vertices[1::9, 2] = vertices[2::9, 2] = -0.0
    return vertices, facesV, facesN


def strip(m):
    """A regular strip of identical triangles over shared vertices: every area ties."""
    vertices = np.zeros((m + 2, 4), np.float32)
    vertices[:, 0] = np.arange(m + 2) // 2
    vertices[:, 1] = np.arange(m + 2) % 2
    facesV = np.zeros((m, 4), np.uint32)
    facesV[:, 0], facesV[:, 1], facesV[:, 2] = np.arange(m), np.arange(m) + 1, np.arange(m) + 2
    return vertices, facesV, normals_for(m, 3)


def grid(side):
    """side x side unit quads in the plane y = 1, two triangles each: 2 side^2 faces, every area ties."""
    x, z = np.meshgrid(np.arange(side + 1), np.arange(side + 1), indexing="ij")
    vertices = np.zeros(((side + 1) ** 2, 4), np.float32)
    vertices[:, 0], vertices[:, 1], vertices[:, 2] = x.ravel(), 1.0, z.ravel()
    i, k = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    a = (i * (side + 1) + k).ravel()
    b, c, d = a + 1, a + side + 1, a + side + 2
    facesV = np.zeros((2 * side * side, 4), np.uint32)
    facesV[0::2, :3] = np.stack([a, b, c], 1)
    facesV[1::2, :3] = np.stack([b, d, c], 1)
    return vertices, facesV, normals_for(facesV.shape[0], 4)


def concentric(m):
    """Triangles of growing size whose boxes all have the origin as their centre: no extent on any axis, every code 0."""
    s = (0.125 * (1 + np.arange(m)))[:, None]
    corners = np.stack([s * [-1, -1, -1], s * [1, -1, 1], s * [0, 1, 0]], 1)
    return _faces(corners, 5)


def repeated(m):
    """One face m times over the same three vertices."""
    vertices = np.array([[0.25, 0.5, 0.75, 0], [1.25, 0.5, 0.5, 0], [0.5, 1.5, 1.0, 0]], np.float32)
    facesV = np.zeros((m, 4), np.uint32)
    facesV[:, :3] = [0, 1, 2]
    return vertices, facesV, normals_for(m, 6)


def wide(m, seed=7):
    """Coordinates in [-1000, 1000] on both sides of 0, 1e-3-sized triangles and one the size of a wall.  The NEGATIVE
    centroids are what holds the sign map of atomicMinFloat / atomicMaxFloat (a map that orders negative floats the wrong way
    moves the bounds and so the cells); the few coordinates at exactly -0.0 only have to do no harm."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1000.0, 1000.0, (m, 1, 3))
    corners = centre + rng.uniform(-5e-4, 5e-4, (m, 3, 3))
    corners[m // 2] = [[-900.0, -900.0, 10.0], [900.0, -900.0, 10.0], [0.0, 900.0, 10.0]]
    corners[0:m:17, 0, 0] = -0.0
    corners[5:m:23, :, 1] = -0.0                                          # whole faces at y = -0.0: a -0.0 centroid
    vertices, facesV, facesN = _faces(corners, seed)
    assert (vertices[:, :3] < 0).any() and (vertices[:, :3] > 0).any() and np.signbit(vertices[vertices == 0]).any()
    return vertices, facesV, facesN


def skew(m, seed=8):
    """m / 2 boxes, each as two identical faces (so a leaf of either builder is one box), of extents (a, b, c) in a random order over the axes, a and b random, c the multiple of 2^-23 that brings
    a b + b c + c a nearest to 1; origins and extents on a 2^-23 grid in [0, 2), so every corner and extent is exact in
    binary32.  The faces' half areas are all within a few units in the last place of 1, so which child goes first turns on
    the order in which (x * y + z * y) + x * z is rounded: another association or a contracted multiply-add shows here."""
    rng = np.random.default_rng(seed)
    m //= 2
    a, b = rng.integers(1 << 15, 1 << 16, (2, m)) / 65536.0                # [0.5, 1) on a 2^-16 grid
    c = np.round((1.0 - a * b) / (a + b) * (1 << 23)) / (1 << 23)           # (0, 0.75]
    d = np.stack([a, b, c], 1)
    d = np.take_along_axis(d, np.argsort(rng.random((m, 3)), 1), 1)
    o = rng.integers(0, 1 << 23, (m, 3)) / float(1 << 23)
    corners = np.repeat(np.stack([o, o + d * [1, 1, 0], o + d * [0, 1, 1]], 1), 2, 0)
    vertices, facesV, facesN = _faces(corners, seed)
    assert np.array_equal(vertices[:, :3].astype(np.float64).reshape(2 * m, 3, 3), corners)
    assert np.array_equal((corners.max(1) - corners.min(1))[::2], d) and np.array_equal(d.astype(np.float32), d)
    return vertices, facesV, facesN


SOUP_SIZES = (255, 256, 257, 300, 513, 769)
TINY_SIZES = (1, 2, 3, 4, 5, 7)
SCENES = (("cornell", 0), ("sponza", 6000), ("hairball", 3001))

# name -> builder of the case, at the sizes the GPU sees
FULL = {"soup-%d" % m: (lambda m=m: soup(m)) for m in SOUP_SIZES}
FULL.update({"strip-257": lambda: strip(257), "grid-512": lambda: grid(16), "flat-300": lambda: flat(300),
             "concentric-40": lambda: concentric(40), "repeated-40": lambda: repeated(40), "wide-300": lambda: wide(300),
             "permuted-257": lambda: permuted(257), "skew-120": lambda: skew(120)})
FULL.update({"tiny-%d" % m: (lambda m=m: soup(m, 9)) for m in TINY_SIZES})

# the same families at <= 96 faces, for the thread-by-thread transcription
SMALL = {"soup-96": lambda: soup(96), "soup-61": lambda: soup(61, 3), "strip-65": lambda: strip(65), "grid-72": lambda: grid(6),
         "flat-80": lambda: flat(80), "concentric-40": lambda: concentric(40), "repeated-40": lambda: repeated(40),
         "wide-90": lambda: wide(90), "permuted-77": lambda: permuted(77), "skew-60": lambda: skew(60)}
SMALL.update({"tiny-%d" % m: (lambda m=m: soup(m, 9)) for m in TINY_SIZES})


def scene(pbr, kind, triangles):
    """The generated scene the existing build test uses (seed 5)."""
    pbr.cfg_reset()
    arr = pbr.HostScene.generate(kind, 5, triangles).arrays()
    return arr["vertices"], arr["facesV"], arr["facesN"]


def small_scene(pbr, kind, faces=96):
    """Every k-th face of the smallest scene of that kind the generator makes (it does not go below some thousand faces), k
    the least that leaves at most `faces`: the kind's walls, columns or strands, thinned out, over its own vertex array."""
    pbr.cfg_reset()
    arr = pbr.HostScene.generate(kind, 5, 90).arrays()
    step = -(-arr["facesV"].shape[0] // faces)
    return arr["vertices"], arr["facesV"][::step].copy(), arr["facesN"][::step].copy()
