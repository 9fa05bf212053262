"""The scenes of the refit tests: the committed fixtures of tests/golden/ as (arrays, desc, config, camera), and the same
scene with other vertices and nodes (S' of include/pbr_hip.h, pbr_update_vertices)."""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_reference_scenes  # noqa: E402

# the procedural fixtures (tests/golden/make_golden.py, CASES): kind, seed, triangles, Cfg overrides, width, height, frames
GENERATED = {
    "cornell_sa": ("cornell", 1, 0, {"render.max_depth": 4}, 32, 32, 2),
    "cornell_schlick": ("cornell", 1, 0, {"render.max_depth": 4, "render.brdf": 0}, 32, 32, 2),
    "cornell_2spp": ("cornell", 1, 0, {"render.samples": 2}, 32, 24, 2),
    "sponza_small": ("sponza", 2, 3000, {}, 32, 24, 1),
    "hairball_small": ("hairball", 3, 2000, {}, 24, 24, 1),
}
REFERENCE = ("ref_pillars_sa", "ref_pillars_schlick", "ref_spheres_sa", "ref_spheres_schlick", "ref_suzanne_sa", "ref_suzanne_sa_shadow",
             "ref_suzanne_schlick", "ref_suzanne_schlick_shadow")
NAMES = REFERENCE + tuple(sorted(GENERATED))
ARRAYS = ("bvh", "facesV", "facesN", "vertices", "normals", "materials", "lights")


class Scene:
    def __init__(self, pbr, arrays, cfg, cam, px, seeds):
        self.pbr, self.arrays, self.cfg, self.cam, self.px, self.seeds = pbr, arrays, cfg, cam, px, seeds
        self.desc = self._desc(arrays)

    def _desc(self, a):
        d = self.pbr.SceneDesc()
        d.bvh, d.num_nodes = a["bvh"].ctypes.data, a["bvh"].shape[0]
        d.facesV, d.facesN, d.num_faces = a["facesV"].ctypes.data, (a["facesN"].ctypes.data if a["facesN"].shape[0] else None), a["facesV"].shape[0]
        d.vertices, d.num_vertices = a["vertices"].ctypes.data, a["vertices"].shape[0]
        d.normals, d.num_normals = (a["normals"].ctypes.data if a["normals"].shape[0] else None), a["normals"].shape[0]
        d.materials, d.num_materials = a["materials"].ctypes.data, a["materials"].shape[0]
        d.brdf = 0 if a["materials"].shape[1] == 12 else 1
        d.lights, d.num_lights = (a["lights"].ctypes.data, a["lights"].shape[0]) if a["lights"].shape[0] else (None, 0)
        return d

    def moved(self, vertices, bvh):
        """S': this scene with other vertices and nodes."""
        a = dict(self.arrays)
        a["vertices"], a["bvh"] = np.ascontiguousarray(vertices, np.float32), np.ascontiguousarray(bvh, np.float32)
        return Scene(self.pbr, a, self.cfg, self.cam, self.px, self.seeds)

    def config(self, **fields):
        cfg = self.pbr.Config.from_buffer_copy(self.cfg)
        for k, v in fields.items():
            setattr(cfg, k, v)
        return cfg


def load(pbr, name):
    if name in GENERATED:
        kind, seed, triangles, overrides, w, h, frames = GENERATED[name]
        pbr.cfg_reset()
        pbr.cfg_set(**overrides)
        sc = pbr.HostScene.generate(kind, seed, triangles)
        cfg, cam, px = sc.config(w, h), sc.camera(), pbr.pixel_dimension(w, h)
        pbr.cfg_reset()
        arrays = sc.arrays()
        arrays["lights"] = arrays["lights"][: sc.desc.num_lights]
        return Scene(pbr, {k: np.ascontiguousarray(arrays[k]) for k in ARRAYS}, cfg, cam, px, pbr.frame_seeds(0, frames))
    data = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    _, cfg, cam, keep = make_reference_scenes.scene_from_fixture(pbr, data)
    return Scene(pbr, {k: keep[k] for k in ARRAYS}, cfg, cam, float(data["px_dim"]), np.asarray(data["seeds"], np.float32))


def generated(pbr, kind, seed, triangles, w, h, **overrides):
    """A procedural scene of host/scene_gen.cpp at any size."""
    pbr.cfg_reset()
    pbr.cfg_set(**overrides)
    sc = pbr.HostScene.generate(kind, seed, triangles)
    cfg, cam, px = sc.config(w, h), sc.camera(), pbr.pixel_dimension(w, h)
    pbr.cfg_reset()
    arrays = sc.arrays()
    arrays["lights"] = arrays["lights"][: sc.desc.num_lights]
    return Scene(pbr, {k: np.ascontiguousarray(arrays[k]) for k in ARRAYS}, cfg, cam, px, pbr.frame_seeds(0, 2))
