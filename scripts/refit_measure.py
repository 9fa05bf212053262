"""pbr_update_vertices timed on one GPU against the alternatives, for one scene per process.

  python scripts/refit_measure.py --scene sponza|dragon|hairball [--reps 7] [--frames 16] [--out FILE]

The BASELINE scenes as bench.py generates them (Sponza-class 260k, Dragon-class 870k, hairball 2M triangles), 1920 x 1080.  The
vertices are moved with tests/refit_ref.py's seeded deformation at its two amplitudes.  Reported, medians over --reps with the
spread (min .. max), wall times around the synchronous calls:
  (a) pbr_update_vertices: device time of its kernels (pbr_last_kernel_ms), the copy of the vertices (pbr_diag_refit_info) and
      the wall time of the call
  (b) the alternatives on the same machine and build: pbr_upload_scene( S' ) alone (S' = the moved vertices + the refitted
      nodes), and pbr_build_bvh + pbr_upload_scene
  (c) the refit's device time against its traffic floor: 16 B per vertex and per face index read, 48 B per face record, 24 B per
      node and, where face normals are kept, 16 B per face written (and the 48 B read back for them) — bytes, GB/s, and the
      fraction of 8 TB/s
  (d) the cost of a stale tree: Msamples/s of pbr_render( --frames ) on the refitted tree against the tree pbr_build_bvh
      builds for the moved vertices, at both amplitudes, the same pinned plan.  (The tree host/bvh_builder.cpp builds for moved
      vertices needs a loader path for arrays that the host library does not have; that leg is not in this script.)
Append the output of the three scenes to profiles/r09/experiments/refit.txt.

  python scripts/refit_measure.py --scene ... --phong ALPHA [--reps 7] [--out FILE]

pbr_update_geometry under Phong tessellation instead (profiles/r14/experiments/patch_refit.txt).  The scene's own vertex normals
are used when most faces have unequal ones; otherwise smooth normals are made (the area-weighted mean of the faces around a
vertex, facesN = facesV).  Positions move as above, normals with tests/patch_refit_ref.py's seeded perturbation.  Reported:
  (a) pbr_update_geometry( V', N' ) with phong_tessellation = ALPHA configured: device time, the copy of vertices + normals, wall
  (b) the same scene's pbr_update_vertices( V' ) with Phong tessellation off: the flat refit — the difference is the price of the
      patches and the thick boxes
  (c) pbr_upload_scene( S' ) + pbr_configure, wall: the only way to move Phong geometry without pbr_update_geometry
  (d) the traffic floor next to (a): the flat refit's, plus 96 B per face of patch records written, 16 B per normal and 16 B per
      face of normal indices read; the 24 B per face of thick boxes written and read again are listed beside it

  python scripts/refit_measure.py --scene ... --transforms [--phong 0.6] [--reps 7] [--out FILE]

pbr_update_transforms (profiles/r15/experiments/transforms.txt), under the --phong leg's conditions: smooth normals made here,
phong_tessellation configured.  The scene is cut into parts by connected component (tests/transform_ref.py); part 0 stays where it is, every other part gets a rotation about the y axis and a translation of its
own, so V' and N' are different arrays for the two calls that are compared on the same context, library and run:
  (a) pbr_update_transforms( M ): device time of the whole update, of the transform kernels alone, the enqueue of the record
      copy, wall
  (b) pbr_update_geometry( V', N' ) with the same V', N' precomputed on the host (not timed): device, copy, wall — the baseline
  (c) wall - device of both: what a caller pays beyond the kernels.  The statement to support or refute: (a)'s wall time comes
      down to its device time plus the flag read-back and the launch cost
  (d) the transform kernels against their traffic floor, 36 B per vertex and per normal

  python scripts/refit_measure.py --scene ... --skin [--phong 0.6] [--reps 9] [--out FILE]

pbr_update_skin (profiles/r16/experiments/skin.txt), under the --transforms leg's conditions and with its matrices.  The bones are
the scene's connected components plus one bone nobody uses; the influences are tests/skin_ref.py's influences_for — one-hot
elements, blends of two, three and four bones, weights that do not sum to 1.  Parts are set on the same context beside the skin.
One warm-up round of all three calls, then the three alternate on the same context in the same run:
  (a) pbr_update_skin( M ): device time of the whole update, of the skin kernels alone, wall
  (b) pbr_update_geometry( V', N' ) with the same V', N' precomputed on the host (not timed): device, copy, wall
  (c) pbr_update_transforms with the one-hot equivalent — every element follows its own part only —: device, its transform
      kernels, wall
  (d) the skin kernels against their traffic floor, 64 B per vertex and per normal (the bone records are not in it)

  python scripts/refit_measure.py --scene ... --morph [--phong 0.6] [--reps 9] [--out FILE]

pbr_update_morph and pbr_update_pose (profiles/r17/experiments/morph.txt), under the --skin leg's conditions, its skin and its
matrices.  Four sets of targets in one run: 8 and 64 targets, each target naming either about 5 % of the vertices — one window
of consecutive indices at a seeded offset, as a blend shape names a region of a mesh — or all of them; normal targets over the
same indices.  Every weight is non-zero: every entry is active.  Per set, one warm-up round, then the four calls alternate on the
same context:
  (a) pbr_update_morph( w ): device time of the whole update, of the morph kernels alone, wall
  (b) pbr_update_pose( w, M ): the same for the pose kernels
  (c) pbr_update_geometry( V', N' ) with the morph's V', N' precomputed on the host (not timed): device, copy, wall
  (d) pbr_update_skin( M ) alone: device, its skin kernels, wall
  (e) the kernels' bytes over their time against the stated traffic: 36 B per element (rest quad, one run word, store) and 16 B
      per entry for the morph, 32 B per element more for the pose (the influence record), 64 B per element for the skin; the
      weight table and the bone records are not in it

  python scripts/refit_measure.py --scene ... --skin-dq [--phong 0.6] [--reps 9] [--out FILE]

pbr_update_skin_dq and pbr_update_pose_dq (profiles/r19/experiments/skin_dq.txt), next to the --skin leg's calls in the same run:
the same scenes, influences and bones, the bones' dual quaternions made by pbr_dual_quats_from_matrices from the leg's rigid
matrices; for the pose the --morph leg's first set of targets (8 of 5 % each).  One warm-up round, then the four calls alternate
on the same context:
  (a) pbr_update_skin_dq( Q ): device time of the whole update, of the dq kernels alone (pbr_diag_skin_dq_info), wall
  (b) pbr_update_pose_dq( w, Q ): the same
  (c) pbr_update_skin( M ) with the same bones as matrices: device, its skin kernels, wall
  (d) pbr_update_geometry( V', N' ) with the dq skin's V', N' precomputed on the host (not timed): device, copy, wall
  (e) (a) against (c) in percent, wall and kernels
  (f) both kernels against the 64 B per element they share (the bone records, 32 against 48 B per active slot, are not in it)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import pbr_loader  # noqa: E402

W, H = 1920, 1080
SCENES = {"dragon": ("dragon", 1, 870000), "sponza": ("sponza", 2, 260000), "hairball": ("hairball", 3, 2000000)}
HBM_BYTES_PER_S = 8.0e12


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def spread(values):
    return "%9.3f (%.3f .. %.3f)" % (float(np.median(values)), min(values), max(values))


def wall(call):
    start = time.perf_counter()
    call()
    return (time.perf_counter() - start) * 1e3


def smooth_normals(facesV, vertices):
    """(facesN, normals): one normal per vertex, the normalised sum of the cross products of the faces around it."""
    f = facesV[:, :3].astype(np.int64)
    v = vertices[:, :3].astype(np.float64)
    cross = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    total = np.zeros_like(v)
    for k in range(3):
        np.add.at(total, f[:, k], cross)
    length = np.linalg.norm(total, axis=1, keepdims=True)
    normals = np.zeros((vertices.shape[0], 4), np.float32)
    normals[:, :3] = np.where(length > 0, total / np.where(length > 0, length, 1.0), [0.0, 1.0, 0.0])
    facesN = np.ascontiguousarray(facesV.copy())
    facesN[:, 3] = 0
    return facesN, normals


def measure_phong(pbr, name, alpha, reps):
    import patch_refit_ref
    import refit_ref
    kind, seed, triangles = SCENES[name]
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 3})
    sc = pbr.HostScene.generate(kind, seed, triangles)
    a = {k: np.ascontiguousarray(v) for k, v in sc.arrays().items()}
    flat_cfg, cam, px = sc.config(W, H), sc.camera(), pbr.pixel_dimension(W, H)
    cfg = pbr.Config.from_buffer_copy(flat_cfg)
    cfg.phong_tessellation = alpha
    faces, vertices, nodes = a["facesV"].shape[0], a["vertices"].shape[0], a["bvh"].shape[0]

    def curved(facesN, normals):
        n = normals[facesN[:, :3].astype(np.int64), :3]
        t = (n[:, 0] - n[:, 1]) + (n[:, 1] - n[:, 2])
        return int((np.abs(t) > np.float32(0.000001)).any(axis=1).sum())

    facesN, normals, source = a["facesN"], a["normals"], "the scene's own normals"
    usable = normals.shape[0] > 0 and facesN.shape[0] == faces and int(facesN[:, :3].max()) < normals.shape[0]
    if not usable or 2 * curved(facesN, normals) < faces:
        facesN, normals = smooth_normals(a["facesV"], a["vertices"])
        source = "smooth normals made here (facesN = facesV)"
    lines = ["== %s under Phong tessellation %g: %d faces (%d with unequal normals), %d vertices, %d normals, %d nodes; %s"
             % (name, alpha, faces, curved(facesN, normals), vertices, normals.shape[0], nodes, source)]

    def desc_with(v, n, bvh):
        d = pbr.SceneDesc.from_buffer_copy(sc.desc)
        d.vertices, d.bvh, d.num_nodes = v.ctypes.data, bvh.ctypes.data, bvh.shape[0]
        d.facesN, d.normals, d.num_normals = facesN.ctypes.data, n.ctypes.data, n.shape[0]
        return d

    dev, flat = pbr.Device(0), pbr.Device(0)
    dev.upload_scene(desc_with(a["vertices"], normals, a["bvh"]))
    dev.configure(cfg)
    flat.upload_scene(desc_with(a["vertices"], normals, a["bvh"]))
    flat.configure(flat_cfg)
    dev.update_geometry(a["vertices"], normals)                      # the first call makes the tables
    lines.append("tables: %d bytes for the patch refit beside the refit's %d" % (dev.patch_refit_info()["device_bytes"], dev.refit_info()["device_bytes"]))
    for amp in refit_ref.AMPLITUDES:
        v = refit_ref.deform(a["facesV"], a["vertices"], amp, seed=3)
        n = patch_refit_ref.perturb_normals(normals, seed=3)
        device_ms, copy_ms, wall_ms, flat_device_ms, flat_wall_ms = [], [], [], [], []
        for _ in range(reps):
            dev.update_geometry(a["vertices"], normals)
            wall_ms.append(wall(lambda: dev.update_geometry(v, n)))
            device_ms.append(dev.last_kernel_ms())
            copy_ms.append(dev.refit_info()["upload_ms"])
            flat.update_vertices(a["vertices"])
            flat_wall_ms.append(wall(lambda: flat.update_vertices(v)))
            flat_device_ms.append(flat.last_kernel_ms())
        lines.append("(a) %-5s update_geometry, phong %g: device %s ms | copy %s ms | wall %s ms" % (amp, alpha, spread(device_ms), spread(copy_ms), spread(wall_ms)))
        lines.append("(b) %-5s update_vertices, phong off: device %s ms | wall %s ms" % (amp, spread(flat_device_ms), spread(flat_wall_ms)))
        refitted = dev.read_bvh()                                        # kept alive: the descriptor only points at it
        moved = desc_with(v, n, refitted)
        other = pbr.Device(0)

        def fresh():
            other.upload_scene(moved)
            other.configure(cfg)
        upload = [wall(fresh) for _ in range(reps)]
        other.close()
        lines.append("(c) %-5s upload_scene( S' ) + configure: wall %s ms" % (amp, spread(upload)))
        face_normals = 1 if dev.scene_bytes()["faces"] else 0
        refit_floor = 16 * vertices + 16 * faces + 48 * faces + 24 * nodes + face_normals * (48 + 16) * faces
        floor = refit_floor + 96 * faces + 16 * normals.shape[0] + 16 * faces
        rate = floor / (float(np.median(device_ms)) * 1e-3)
        lines.append("(d) %-5s traffic floor %d bytes (the flat refit's %d) -> %.1f GB/s = %.1f %% of 8 TB/s; thick boxes, written and read again: %d bytes more"
                     % (amp, floor, refit_floor, rate / 1e9, 100.0 * rate / HBM_BYTES_PER_S, 48 * faces))
    dev.close()
    flat.close()
    return lines


def measure_transforms(pbr, name, alpha, reps):
    import transform_ref
    kind, seed, triangles = SCENES[name]
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 3})
    sc = pbr.HostScene.generate(kind, seed, triangles)
    a = {k: np.ascontiguousarray(v) for k, v in sc.arrays().items()}
    cfg = sc.config(W, H)
    cfg.phong_tessellation = alpha
    faces, vertices = a["facesV"].shape[0], a["vertices"].shape[0]
    # normals as in the --phong leg: the BASELINE scenes carry no smooth normals, so one per vertex is made (facesN = facesV)
    facesN, normals = smooth_normals(a["facesV"], a["vertices"])
    count = normals.shape[0]
    desc = pbr.SceneDesc.from_buffer_copy(sc.desc)
    desc.facesN, desc.normals, desc.num_normals = facesN.ctypes.data, normals.ctypes.data, count
    dev = pbr.Device(0)
    dev.upload_scene(desc)
    dev.configure(cfg)
    assert dev.patch_refit_info()["patches"]
    vertex_part, normal_part, parts = transform_ref.parts_of(name, a["facesV"], facesN, vertices, count)
    lines = ["== %s by transforms, phong_tessellation %g: %d faces, %d vertices, %d smooth normals made here (facesN = facesV), %d parts by connected component"
             % (name, alpha, faces, vertices, count, parts)]
    dev.set_parts(vertex_part, normal_part, parts)
    lines.append("tables: %d bytes for the parts beside the refit's %d and the patch refit's %d"
                 % (dev.transform_info()["device_bytes"], dev.refit_info()["device_bytes"], dev.patch_refit_info()["device_bytes"]))
    rest_n = normals

    def matrices(step):
        """Part 0 the identity; part k turned about y by an angle of its own and shifted a little, another pose per step."""
        k = np.arange(parts, dtype=np.float64)
        angle = 0.05 * step + 0.001 * (k % 97)
        m = np.zeros((parts, 3, 4))
        m[:, 0, 0], m[:, 0, 2], m[:, 2, 0], m[:, 2, 2], m[:, 1, 1] = np.cos(angle), np.sin(angle), -np.sin(angle), np.cos(angle), 1.0
        m[:, :, 3] = 0.01 * step * np.stack([np.cos(k), np.sin(k), np.cos(2.0 * k)], axis=1)
        m[0] = np.eye(3, 4)
        return np.ascontiguousarray(m.reshape(parts, 12), np.float32)

    poses = []
    for step in (1, 2):
        M = matrices(step)
        v, n = transform_ref.transform(a["vertices"], vertex_part, rest_n, normal_part, M)
        poses.append((M, v, n))
    dev.update_transforms(poses[0][0])                               # both paths warm
    dev.update_geometry(poses[0][1], poses[0][2])
    got_v, got_n = None, None
    xf = {key: [] for key in ("device", "kernels", "copy", "wall")}
    geo = {key: [] for key in ("device", "copy", "wall")}
    for rep in range(reps):
        M, v, n = poses[rep % 2]
        xf["wall"].append(wall(lambda: dev.update_transforms(M)))
        xf["device"].append(dev.last_kernel_ms())
        xf["kernels"].append(dev.transform_info()["ms"])
        xf["copy"].append(dev.refit_info()["upload_ms"])
        if rep == 0:
            got_v, got_n = dev.read_geometry()
            same = np.array_equal(got_v.view(np.uint32), v.view(np.uint32)) and (n is None or np.array_equal(got_n.view(np.uint32), n.view(np.uint32)))
            lines.append("read_geometry after the first timed update equals the numpy restatement bit for bit: %s" % same)
        geo["wall"].append(wall(lambda: dev.update_geometry(v, n)))
        geo["device"].append(dev.last_kernel_ms())
        geo["copy"].append(dev.refit_info()["upload_ms"])
    lines.append("(a) update_transforms: device %s ms | transform kernels %s ms | record copy enqueue %s ms | wall %s ms"
                 % (spread(xf["device"]), spread(xf["kernels"]), spread(xf["copy"]), spread(xf["wall"])))
    lines.append("(b) update_geometry( V', N' ): device %s ms | copy %s ms | wall %s ms" % (spread(geo["device"]), spread(geo["copy"]), spread(geo["wall"])))
    lines.append("(c) wall - device, per repetition: update_transforms %s ms | update_geometry %s ms"
                 % (spread([w - d for w, d in zip(xf["wall"], xf["device"])]), spread([w - d for w, d in zip(geo["wall"], geo["device"])])))
    floor = 36 * vertices + 36 * count
    rate = floor / (float(np.median(xf["kernels"])) * 1e-3)
    lines.append("(d) transform kernels: traffic floor %d bytes -> %.1f GB/s = %.1f %% of 8 TB/s" % (floor, rate / 1e9, 100.0 * rate / HBM_BYTES_PER_S))
    dev.close()
    return lines


def measure_skin(pbr, name, alpha, reps):
    import skin_ref
    import transform_ref
    kind, seed, triangles = SCENES[name]
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 3})
    sc = pbr.HostScene.generate(kind, seed, triangles)
    a = {k: np.ascontiguousarray(v) for k, v in sc.arrays().items()}
    cfg = sc.config(W, H)
    cfg.phong_tessellation = alpha
    faces, vertices = a["facesV"].shape[0], a["vertices"].shape[0]
    # normals as in the --phong leg: the BASELINE scenes carry no smooth normals, so one per vertex is made (facesN = facesV)
    facesN, normals = smooth_normals(a["facesV"], a["vertices"])
    count = normals.shape[0]
    desc = pbr.SceneDesc.from_buffer_copy(sc.desc)
    desc.facesN, desc.normals, desc.num_normals = facesN.ctypes.data, normals.ctypes.data, count
    dev = pbr.Device(0)
    dev.upload_scene(desc)
    dev.configure(cfg)
    assert dev.patch_refit_info()["patches"]
    vertex_part, normal_part, parts = transform_ref.parts_of(name, a["facesV"], facesN, vertices, count)
    vb, vw, nb, nw, bones = skin_ref.influences_for(name, a["facesV"], facesN, vertices, count)
    assert bones == parts + 1
    slots = np.bincount((vw != 0).sum(axis=1), minlength=5)[1:]
    lines = ["== %s by a skin, phong_tessellation %g: %d faces, %d vertices, %d smooth normals made here (facesN = facesV), %d bones (the connected components and one nobody uses)"
             % (name, alpha, faces, vertices, count, bones),
             "influences: %d / %d / %d / %d vertices with 1 / 2 / 3 / 4 weights that are not 0 (tests/skin_ref.py, influences_for)" % tuple(slots)]
    dev.set_skin(vb, vw, nb, nw, bones)
    dev.set_parts(vertex_part, normal_part, parts)
    assert dev.skin_info()["device_bytes"] == 64 * vertices + 48 * count + 48 * bones + 4
    lines.append("tables: %d bytes for the skin, %d for the parts, beside the refit's %d and the patch refit's %d"
                 % (dev.skin_info()["device_bytes"], dev.transform_info()["device_bytes"], dev.refit_info()["device_bytes"], dev.patch_refit_info()["device_bytes"]))

    poses = []
    for step in (1, 2):
        M = bone_matrices(bones, step)
        v, n = skin_ref.skin(a["vertices"], vb, vw, normals, nb, nw, M)
        poses.append((M, v, n))
    dev.update_skin(poses[0][0])                                     # all three paths warm
    dev.update_geometry(poses[0][1], poses[0][2])
    dev.update_transforms(poses[0][0][:parts])
    skin = {key: [] for key in ("device", "kernels", "wall")}
    geo = {key: [] for key in ("device", "copy", "wall")}
    xf = {key: [] for key in ("device", "kernels", "wall")}
    for rep in range(reps):
        M, v, n = poses[rep % 2]
        skin["wall"].append(wall(lambda: dev.update_skin(M)))
        skin["device"].append(dev.last_kernel_ms())
        skin["kernels"].append(dev.skin_info()["ms"])
        if rep == 0:
            got_v, got_n = dev.read_geometry()
            same = np.array_equal(got_v.view(np.uint32), v.view(np.uint32)) and np.array_equal(got_n.view(np.uint32), n.view(np.uint32))
            lines.append("read_geometry after the first timed update equals the numpy restatement bit for bit: %s" % same)
        geo["wall"].append(wall(lambda: dev.update_geometry(v, n)))
        geo["device"].append(dev.last_kernel_ms())
        geo["copy"].append(dev.refit_info()["upload_ms"])
        xf["wall"].append(wall(lambda: dev.update_transforms(M[:parts])))
        xf["device"].append(dev.last_kernel_ms())
        xf["kernels"].append(dev.transform_info()["ms"])
    lines.append("(a) update_skin: device %s ms | skin kernels %s ms | wall %s ms" % (spread(skin["device"]), spread(skin["kernels"]), spread(skin["wall"])))
    lines.append("(b) update_geometry( V', N' ): device %s ms | copy %s ms | wall %s ms" % (spread(geo["device"]), spread(geo["copy"]), spread(geo["wall"])))
    lines.append("(c) update_transforms, one-hot: device %s ms | transform kernels %s ms | wall %s ms" % (spread(xf["device"]), spread(xf["kernels"]), spread(xf["wall"])))
    floor = 64 * vertices + 64 * count
    rate = floor / (float(np.median(skin["kernels"])) * 1e-3)
    lines.append("(d) skin kernels: traffic floor %d bytes -> %.1f GB/s = %.1f %% of 8 TB/s" % (floor, rate / 1e9, 100.0 * rate / HBM_BYTES_PER_S))
    dev.close()
    return lines


def bone_matrices(bones, step):
    """Bone 0 the identity; bone k turned about y by an angle of its own and shifted a little, another pose per step (the
    --skin leg's matrices)."""
    k = np.arange(bones, dtype=np.float64)
    angle = 0.05 * step + 0.001 * (k % 97)
    m = np.zeros((bones, 3, 4))
    m[:, 0, 0], m[:, 0, 2], m[:, 2, 0], m[:, 2, 2], m[:, 1, 1] = np.cos(angle), np.sin(angle), -np.sin(angle), np.cos(angle), 1.0
    m[:, :, 3] = 0.01 * step * np.stack([np.cos(k), np.sin(k), np.cos(2.0 * k)], axis=1)
    m[0] = np.eye(3, 4)
    return np.ascontiguousarray(m.reshape(bones, 12), np.float32)


def measure_skin_dq(pbr, name, alpha, reps):
    import skin_dq_ref
    import skin_ref
    kind, seed, triangles = SCENES[name]
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 3})
    sc = pbr.HostScene.generate(kind, seed, triangles)
    a = {k: np.ascontiguousarray(v) for k, v in sc.arrays().items()}
    cfg = sc.config(W, H)
    cfg.phong_tessellation = alpha
    faces, vertices = a["facesV"].shape[0], a["vertices"].shape[0]
    facesN, normals = smooth_normals(a["facesV"], a["vertices"])
    count = normals.shape[0]
    desc = pbr.SceneDesc.from_buffer_copy(sc.desc)
    desc.facesN, desc.normals, desc.num_normals = facesN.ctypes.data, normals.ctypes.data, count
    vb, vw, nb, nw, bones = skin_ref.influences_for(name, a["facesV"], facesN, vertices, count)
    extent = float(np.abs(a["vertices"][:, :3]).max())
    # the --morph leg's first set: 8 targets, each a window of 5 % of the elements
    rng = np.random.default_rng(17 * 8 + 5)
    vt, nt = [], []
    for _ in range(8):
        for out, n, size in ((vt, vertices, 0.002 * extent), (nt, count, 0.05)):
            window = max(1, int(0.05 * n))
            index = ((int(rng.integers(0, n)) + np.arange(window)) % n).astype(np.uint32)
            out.append((index, (rng.random((window, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(2.0 * size)))
    dev = pbr.Device(0)
    dev.upload_scene(desc)
    dev.configure(cfg)
    dev.set_skin(vb, vw, nb, nw, bones)
    dev.set_morph(vt, nt)
    lines = ["== %s by a dual-quaternion skin, phong_tessellation %g: %d faces, %d vertices, %d smooth normals made here (facesN = facesV), %d bones; the --skin leg's "
             "influences and matrices, the bones' dual quaternions by pbr_dual_quats_from_matrices; 8 morph targets of 5 %% each for the pose"
             % (name, alpha, faces, vertices, count, bones),
             "tables: %d bytes for the skin with or without dual quaternions, %d for the morph" % (dev.skin_info()["device_bytes"], dev.morph_info()["device_bytes"])]
    poses = []
    for step in (1, 2):
        M = bone_matrices(bones, step)
        Q = pbr.dual_quats_from_matrices(M)
        w = ((0.1 + 0.01 * np.arange(8)) * np.where(np.arange(8) % 2 == 0, 1.0, -1.0) * step).astype(np.float32)
        v, n = skin_dq_ref.skin(a["vertices"], vb, vw, normals, nb, nw, Q)
        poses.append((M, Q, w, v, n))
    M, Q, w, v, n = poses[0]
    dev.update_skin(M)                                               # all four paths warm
    dev.update_skin_dq(Q)
    dev.update_pose_dq(w, Q)
    dev.update_geometry(v, n)
    skin = {key: [] for key in ("device", "kernels", "wall")}
    dq = {key: [] for key in ("device", "kernels", "wall")}
    pose = {key: [] for key in ("device", "kernels", "wall")}
    geo = {key: [] for key in ("device", "copy", "wall")}
    for rep in range(reps):
        M, Q, w, v, n = poses[rep % 2]
        skin["wall"].append(wall(lambda: dev.update_skin(M)))
        skin["device"].append(dev.last_kernel_ms())
        skin["kernels"].append(dev.skin_info()["ms"])
        dq["wall"].append(wall(lambda: dev.update_skin_dq(Q)))
        dq["device"].append(dev.last_kernel_ms())
        dq["kernels"].append(dev.skin_dq_info()["ms"])
        if rep == 0:
            got_v, got_n = dev.read_geometry()
            same = np.array_equal(got_v.view(np.uint32), v.view(np.uint32)) and np.array_equal(got_n.view(np.uint32), n.view(np.uint32))
            lines.append("read_geometry after the first timed update_skin_dq equals the numpy restatement bit for bit: %s" % same)
        pose["wall"].append(wall(lambda: dev.update_pose_dq(w, Q)))
        pose["device"].append(dev.last_kernel_ms())
        pose["kernels"].append(dev.skin_dq_info()["ms"])
        if rep == 0:
            got_v, got_n = dev.read_geometry()
            want_v, want_n = skin_dq_ref.pose(a["vertices"], vt, vb, vw, normals, nt, nb, nw, w, Q)
            same = np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)) and np.array_equal(got_n.view(np.uint32), want_n.view(np.uint32))
            lines.append("read_geometry after the first timed update_pose_dq equals the numpy restatement bit for bit: %s" % same)
        geo["wall"].append(wall(lambda: dev.update_geometry(v, n)))
        geo["device"].append(dev.last_kernel_ms())
        geo["copy"].append(dev.refit_info()["upload_ms"])
    lines.append("(a) update_skin_dq: device %s ms | dq kernels %s ms | wall %s ms" % (spread(dq["device"]), spread(dq["kernels"]), spread(dq["wall"])))
    lines.append("(b) update_pose_dq: device %s ms | dq kernels %s ms | wall %s ms" % (spread(pose["device"]), spread(pose["kernels"]), spread(pose["wall"])))
    lines.append("(c) update_skin, the same bones as matrices: device %s ms | skin kernels %s ms | wall %s ms" % (spread(skin["device"]), spread(skin["kernels"]), spread(skin["wall"])))
    lines.append("(d) update_geometry( V', N' ): device %s ms | copy %s ms | wall %s ms" % (spread(geo["device"]), spread(geo["copy"]), spread(geo["wall"])))
    lines.append("(e) update_skin_dq against update_skin, medians: wall %+.1f %% | kernels %+.1f %%"
                 % (100.0 * (np.median(dq["wall"]) / np.median(skin["wall"]) - 1.0), 100.0 * (np.median(dq["kernels"]) / np.median(skin["kernels"]) - 1.0)))
    floor = 64 * vertices + 64 * count
    for label, times in (("dq", dq["kernels"]), ("skin", skin["kernels"])):
        rate = floor / (float(np.median(times)) * 1e-3)
        lines.append("(f) %s kernels: traffic floor %d bytes -> %.1f GB/s = %.1f %% of 8 TB/s" % (label, floor, rate / 1e9, 100.0 * rate / HBM_BYTES_PER_S))
    dev.close()
    return lines


def measure_morph(pbr, name, alpha, reps):
    import morph_ref
    import skin_ref
    kind, seed, triangles = SCENES[name]
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 3})
    sc = pbr.HostScene.generate(kind, seed, triangles)
    a = {k: np.ascontiguousarray(v) for k, v in sc.arrays().items()}
    cfg = sc.config(W, H)
    cfg.phong_tessellation = alpha
    faces, vertices = a["facesV"].shape[0], a["vertices"].shape[0]
    facesN, normals = smooth_normals(a["facesV"], a["vertices"])
    count = normals.shape[0]
    desc = pbr.SceneDesc.from_buffer_copy(sc.desc)
    desc.facesN, desc.normals, desc.num_normals = facesN.ctypes.data, normals.ctypes.data, count
    vb, vw, nb, nw, bones = skin_ref.influences_for(name, a["facesV"], facesN, vertices, count)
    extent = float(np.abs(a["vertices"][:, :3]).max())
    lines = ["== %s by a morph, phong_tessellation %g: %d faces, %d vertices, %d smooth normals made here (facesN = facesV), %d bones"
             % (name, alpha, faces, vertices, count, bones)]
    dev = pbr.Device(0)
    for targets, cover in ((8, 0.05), (8, 1.0), (64, 0.05), (64, 1.0)):
        rng = np.random.default_rng(17 * targets + int(100 * cover))
        vt, nt = [], []
        for _ in range(targets):
            for out, n, size in ((vt, vertices, 0.002 * extent), (nt, count, 0.05)):
                window = n if cover >= 1.0 else max(1, int(cover * n))
                index = ((int(rng.integers(0, n)) + np.arange(window)) % n).astype(np.uint32)
                out.append((index, (rng.random((window, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(2.0 * size)))
        ev, en = sum(t[0].size for t in vt), sum(t[0].size for t in nt)
        runs = np.bincount(np.concatenate([t[0] for t in vt]), minlength=vertices)
        dev.upload_scene(desc)                                       # a fresh rest pose for every set
        dev.configure(cfg)
        dev.set_skin(vb, vw, nb, nw, bones)
        dev.set_morph(vt, nt)
        info = dev.morph_info()
        assert info["device_bytes"] == morph_ref.expected_bytes(vertices, vt, count, nt) and info["vertex_entries"] == ev and info["normal_entries"] == en
        lines.append("-- %d targets, each naming %s: %d vertex entries, %d normal entries; a vertex's run is %d .. %d entries, %.2f on average; %d bytes for the morph beside the skin's %d"
                     % (targets, "every element" if cover >= 1.0 else "a window of %g %% of the elements" % (100.0 * cover), ev, en, runs.min(), runs.max(), runs.mean(),
                        info["device_bytes"], dev.skin_info()["device_bytes"]))
        poses = []
        for step in (1, 2):
            w = ((0.1 + 0.01 * np.arange(targets)) * np.where(np.arange(targets) % 2 == 0, 1.0, -1.0) * step).astype(np.float32)
            v, n = morph_ref.morph(a["vertices"], vt, normals, nt, w)
            poses.append((w, bone_matrices(bones, step), v, n))
        w, M, v, n = poses[0]
        dev.update_morph(w)                                          # all four paths warm
        dev.update_pose(w, M)
        dev.update_geometry(v, n)
        dev.update_skin(M)
        morph = {key: [] for key in ("device", "kernels", "wall")}
        pose = {key: [] for key in ("device", "kernels", "wall")}
        geo = {key: [] for key in ("device", "copy", "wall")}
        skin = {key: [] for key in ("device", "kernels", "wall")}
        for rep in range(reps):
            w, M, v, n = poses[rep % 2]
            morph["wall"].append(wall(lambda: dev.update_morph(w)))
            morph["device"].append(dev.last_kernel_ms())
            morph["kernels"].append(dev.morph_info()["ms"])
            if rep == 0:
                got_v, got_n = dev.read_geometry()
                same = np.array_equal(got_v.view(np.uint32), v.view(np.uint32)) and np.array_equal(got_n.view(np.uint32), n.view(np.uint32))
                lines.append("read_geometry after the first timed update_morph equals the numpy restatement bit for bit: %s" % same)
            pose["wall"].append(wall(lambda: dev.update_pose(w, M)))
            pose["device"].append(dev.last_kernel_ms())
            pose["kernels"].append(dev.morph_info()["ms"])
            geo["wall"].append(wall(lambda: dev.update_geometry(v, n)))
            geo["device"].append(dev.last_kernel_ms())
            geo["copy"].append(dev.refit_info()["upload_ms"])
            skin["wall"].append(wall(lambda: dev.update_skin(M)))
            skin["device"].append(dev.last_kernel_ms())
            skin["kernels"].append(dev.skin_info()["ms"])
        lines.append("(a) update_morph: device %s ms | morph kernels %s ms | wall %s ms" % (spread(morph["device"]), spread(morph["kernels"]), spread(morph["wall"])))
        lines.append("(b) update_pose: device %s ms | pose kernels %s ms | wall %s ms" % (spread(pose["device"]), spread(pose["kernels"]), spread(pose["wall"])))
        lines.append("(c) update_geometry( V', N' ): device %s ms | copy %s ms | wall %s ms" % (spread(geo["device"]), spread(geo["copy"]), spread(geo["wall"])))
        lines.append("(d) update_skin alone: device %s ms | skin kernels %s ms | wall %s ms" % (spread(skin["device"]), spread(skin["kernels"]), spread(skin["wall"])))
        elements = vertices + count
        for label, traffic, times in (("morph", 36 * elements + 16 * (ev + en), morph["kernels"]), ("pose", 68 * elements + 16 * (ev + en), pose["kernels"]),
                                      ("skin", 64 * elements, skin["kernels"])):
            rate = traffic / (float(np.median(times)) * 1e-3)
            lines.append("(e) %s kernels: stated traffic %d bytes -> %.1f GB/s = %.1f %% of 8 TB/s" % (label, traffic, rate / 1e9, 100.0 * rate / HBM_BYTES_PER_S))
    dev.close()
    return lines


def main():
    import refit_ref
    pbr = pbr_loader.load()
    name, reps, frames = arg("--scene", "sponza"), int(arg("--reps", "7")), int(arg("--frames", "16"))
    if "--morph" in sys.argv:
        text = "\n".join(measure_morph(pbr, name, float(arg("--phong", "0.6")), int(arg("--reps", "9")))) + "\n"
        sys.stdout.write(text)
        if "--out" in sys.argv:
            with open(arg("--out", ""), "a") as f:
                f.write(text)
        return
    if "--skin-dq" in sys.argv:
        text = "\n".join(measure_skin_dq(pbr, name, float(arg("--phong", "0.6")), int(arg("--reps", "9")))) + "\n"
        sys.stdout.write(text)
        if "--out" in sys.argv:
            with open(arg("--out", ""), "a") as f:
                f.write(text)
        return
    if "--skin" in sys.argv:
        text = "\n".join(measure_skin(pbr, name, float(arg("--phong", "0.6")), int(arg("--reps", "9")))) + "\n"
        sys.stdout.write(text)
        if "--out" in sys.argv:
            with open(arg("--out", ""), "a") as f:
                f.write(text)
        return
    if "--transforms" in sys.argv:
        text = "\n".join(measure_transforms(pbr, name, float(arg("--phong", "0.6")), reps)) + "\n"
        sys.stdout.write(text)
        if "--out" in sys.argv:
            with open(arg("--out", ""), "a") as f:
                f.write(text)
        return
    if "--phong" in sys.argv:
        text = "\n".join(measure_phong(pbr, name, float(arg("--phong", "0.6")), reps)) + "\n"
        sys.stdout.write(text)
        if "--out" in sys.argv:
            with open(arg("--out", ""), "a") as f:
                f.write(text)
        return
    kind, seed, triangles = SCENES[name]
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 3})
    sc = pbr.HostScene.generate(kind, seed, triangles)
    a = sc.arrays()
    cfg, cam, px = sc.config(W, H), sc.camera(), pbr.pixel_dimension(W, H)
    seeds = pbr.frame_seeds(0, frames)
    faces, vertices, nodes = a["facesV"].shape[0], a["vertices"].shape[0], a["bvh"].shape[0]
    lines = ["== %s: %d faces, %d vertices, %d nodes, %d x %d" % (name, faces, vertices, nodes, W, H)]

    dev = pbr.Device(0)
    dev.upload_scene(sc.desc)
    dev.configure(cfg)
    dev.render(0, pbr.frame_seeds(0, max(frames, dev.tune_budget())), px, cam)
    plan = dev.last_plan()[1]
    plan = plan if plan >= 0 else 4
    dev.pin_plan(plan)
    info = dev.refit_info()
    lines.append("partition: %(workgroups)d workgroups, %(subtrees)d subtrees, %(top_nodes)d nodes above the cut in %(top_levels)d levels; %(device_bytes)d bytes kept" % info)
    moved = {amp: refit_ref.deform(a["facesV"], a["vertices"], amp, seed=3) for amp in refit_ref.AMPLITUDES}

    def desc_with(v, bvh, facesV=None, facesN=None):
        d = pbr.SceneDesc.from_buffer_copy(sc.desc)
        d.vertices, d.bvh, d.num_nodes = v.ctypes.data, bvh.ctypes.data, bvh.shape[0]
        if facesV is not None:
            d.facesV, d.facesN = facesV.ctypes.data, facesN.ctypes.data
        return d

    for amp, v in moved.items():
        device_ms, copy_ms, wall_ms = [], [], []
        for _ in range(reps):
            dev.update_vertices(a["vertices"])
            wall_ms.append(wall(lambda: dev.update_vertices(v)))
            device_ms.append(dev.last_kernel_ms())
            copy_ms.append(dev.refit_info()["upload_ms"])
        lines.append("(a) %-5s update_vertices: device %s ms | vertex copy %s ms | wall %s ms" % (amp, spread(device_ms), spread(copy_ms), spread(wall_ms)))
        normals = 1 if dev.scene_bytes()["faces"] else 0
        floor = 16 * vertices + 16 * faces + 48 * faces + 24 * nodes + normals * (48 + 16) * faces
        rate = floor / (float(np.median(device_ms)) * 1e-3)
        lines.append("(c) %-5s traffic floor %d bytes -> %.1f GB/s = %.1f %% of 8 TB/s" % (amp, floor, rate / 1e9, 100.0 * rate / HBM_BYTES_PER_S))
        refitted = dev.read_bvh()
        dev.reset_accum()
        stale = [wall(lambda: dev.render(0, seeds, px, cam)) for _ in range(reps)]

        other = pbr.Device(0)
        other.configure(cfg)
        other.pin_plan(plan)
        d1 = desc_with(v, refitted)
        upload = [wall(lambda: other.upload_scene(d1)) for _ in range(reps)]
        lines.append("(b) %-5s upload_scene( S' ): wall %s ms" % (amp, spread(upload)))
        build = []
        for _ in range(max(1, reps // 2)):
            start = time.perf_counter()
            built, outV, outN = other.build_bvh(v, a["facesV"], a["facesN"])
            d2 = desc_with(v, built, outV, outN)
            other.upload_scene(d2)
            build.append((time.perf_counter() - start) * 1e3)
        lines.append("(b) %-5s build_bvh + upload_scene: wall %s ms" % (amp, spread(build)))
        other.render(0, seeds, px, cam)
        fresh = [wall(lambda: other.render(0, seeds, px, cam)) for _ in range(reps)]
        samples = W * H * frames * cfg.samples / 1e6
        lines.append("(d) %-5s render( %d ) plan %d: refitted tree %.1f Msamples/s | tree built for V' by pbr_build_bvh %.1f Msamples/s (wall, medians)"
                     % (amp, frames, plan, samples / (np.median(stale) * 1e-3), samples / (np.median(fresh) * 1e-3)))
        other.close()
    dev.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
