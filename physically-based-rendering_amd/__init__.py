"""MI355X path-tracing core behind the sebadorn/Physically-based-Rendering dispatch surface.

Python here is harness glue only (ctypes): the product is

  csrc/libpbrhip.so    hand-written HIP kernels for gfx950 + the C ABI of include/pbr_hip.h
  host/libpbrhost.so   the C++ host side (loaders, BVH builder, buffer packing, PathTracer)

The directory name is not an importable identifier; load it with `pbr_loader.load()` (repo
root), which registers it as module `pbr_amd`.  There is no CPU fallback: if libpbrhip.so is
missing and cannot be built, importing this package raises.
"""
import ctypes
import os

import numpy as np

from . import build as _build
from . import tiles  # noqa: F401  (layout helpers for the multi-GPU path)

_HERE = os.path.dirname(os.path.abspath(__file__))

PBR_OK = 0


class Float4(ctypes.Structure):
    _fields_ = [("x", ctypes.c_float), ("y", ctypes.c_float), ("z", ctypes.c_float), ("w", ctypes.c_float)]


class Camera(ctypes.Structure):
    """pbr_camera / camera_cl (source/PathTracer.h:25-32), 80 bytes."""
    _fields_ = [("eye", Float4), ("w", Float4), ("u", Float4), ("v", Float4),
                ("focusPoint", ctypes.c_int32 * 2), ("lense", ctypes.c_float * 2)]


class DenoiseParams(ctypes.Structure):
    """pbr_denoise_params.  Defaults: what scripts/denoise_demo.py found best around 4 spp (sigma_color: 4.0 at 1 spp,
    0.6 at 16, 0.3 at 64 — the noise it has to bridge shrinks with the sample count)."""
    _fields_ = [("passes", ctypes.c_uint32), ("sigma_color", ctypes.c_float), ("sigma_normal", ctypes.c_float),
                ("sigma_world", ctypes.c_float), ("sigma_albedo", ctypes.c_float)]

    def __init__(self, passes=5, sigma_color=1.2, sigma_normal=0.25, sigma_world=3.0, sigma_albedo=0.1):
        super().__init__(passes, sigma_color, sigma_normal, sigma_world, sigma_albedo)


class GuidedDenoiseParams(ctypes.Structure):
    """pbr_denoise_guided_params.  sigma_luminance is in standard deviations of the pixel's mean (the variance
    pbr_render_adaptive estimates), so one value serves every sample count."""
    _fields_ = [("passes", ctypes.c_uint32), ("sigma_luminance", ctypes.c_float), ("sigma_normal", ctypes.c_float),
                ("sigma_world", ctypes.c_float), ("sigma_albedo", ctypes.c_float)]

    def __init__(self, passes=5, sigma_luminance=4.0, sigma_normal=0.25, sigma_world=3.0, sigma_albedo=0.1):
        super().__init__(passes, sigma_luminance, sigma_normal, sigma_world, sigma_albedo)


class TemporalParams(ctypes.Structure):
    """pbr_temporal_params: the history of pbr_denoise_temporal.  max_history caps the history length (1 = no reuse); a
    history tap counts if its normal's cosine with the pixel's is >= normal_cos and it lies within sigma_world pixel
    footprints of the pixel's first hit (0 switches that term off)."""
    _fields_ = [("max_history", ctypes.c_uint32), ("normal_cos", ctypes.c_float), ("sigma_world", ctypes.c_float)]

    def __init__(self, max_history=32, normal_cos=0.9, sigma_world=3.0):
        super().__init__(max_history, normal_cos, sigma_world)


class SceneDesc(ctypes.Structure):
    """pbr_scene_desc"""
    _fields_ = [
        ("bvh", ctypes.c_void_p), ("num_nodes", ctypes.c_uint32),
        ("facesV", ctypes.c_void_p), ("facesN", ctypes.c_void_p), ("num_faces", ctypes.c_uint32),
        ("vertices", ctypes.c_void_p), ("num_vertices", ctypes.c_uint32),
        ("normals", ctypes.c_void_p), ("num_normals", ctypes.c_uint32),
        ("materials", ctypes.c_void_p), ("num_materials", ctypes.c_uint32),
        ("brdf", ctypes.c_uint32),
        ("lights", ctypes.c_void_p), ("num_lights", ctypes.c_uint32),
    ]


class Config(ctypes.Structure):
    """pbr_config"""
    _fields_ = [
        ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("brdf", ctypes.c_uint32),
        ("shadow_rays", ctypes.c_uint32), ("max_depth", ctypes.c_uint32), ("max_added_depth", ctypes.c_uint32),
        ("samples", ctypes.c_uint32), ("anti_aliasing", ctypes.c_float), ("phong_tessellation", ctypes.c_float),
        ("sky_light", ctypes.c_float * 4), ("tile_world", ctypes.c_uint32), ("tile_rank", ctypes.c_uint32),
        ("traversal", ctypes.c_uint32), ("arith", ctypes.c_uint32),
    ]


class AdaptiveParams(ctypes.Structure):
    """pbr_adaptive_params"""
    _fields_ = [("min_frames", ctypes.c_uint32), ("round_frames", ctypes.c_uint32), ("max_frames", ctypes.c_uint32),
                ("threshold", ctypes.c_float)]


class DisplayParams(ctypes.Structure):
    """pbr_display_params.  exposure_mode 0 manual (exposure) / 1 auto (key, the two trim fractions, the clamp of the log2 mean,
    adapt); curve 0 clamp / 1 extended Reinhard (white) / 2 ACES fit; transfer 0 linear / 1 sRGB.  The defaults: auto exposure to
    a key of 0.18 over the middle 90 % of the lit pixels, jumping to the target, ACES, sRGB."""
    _fields_ = [("exposure_mode", ctypes.c_uint32), ("exposure", ctypes.c_float), ("key", ctypes.c_float),
                ("low_fraction", ctypes.c_float), ("high_fraction", ctypes.c_float), ("min_log2", ctypes.c_float),
                ("max_log2", ctypes.c_float), ("adapt", ctypes.c_float), ("curve", ctypes.c_uint32), ("white", ctypes.c_float),
                ("transfer", ctypes.c_uint32)]

    def __init__(self, exposure_mode=1, exposure=1.0, key=0.18, low_fraction=0.05, high_fraction=0.05, min_log2=-16.0, max_log2=16.0,
                 adapt=1.0, curve=2, white=4.0, transfer=1):
        super().__init__(exposure_mode, exposure, key, low_fraction, high_fraction, min_log2, max_log2, adapt, curve, white, transfer)


class DisplayInfo(ctypes.Structure):
    """pbr_display_info"""
    _fields_ = [("exposure", ctypes.c_float), ("log2_target", ctypes.c_double), ("log2_used", ctypes.c_double),
                ("counted", ctypes.c_uint64), ("dark", ctypes.c_uint64), ("histogram", ctypes.c_uint32 * 256)]


class Counters(ctypes.Structure):
    _fields_ = [("nodes", ctypes.c_uint64), ("tris", ctypes.c_uint64), ("hits", ctypes.c_uint64), ("paths", ctypes.c_uint64)]


def _load(path, builder):
    builder()      # a no-op unless the library is missing or older than its sources (build.py _stale)
    try:
        return ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    except OSError:
        builder(force=True)
        return ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)


try:
    _lab = os.environ.get("PBR_LAB_ENV") == "1"   # lab runs only: no PBR_* variable steers a product process
    if _lab and os.environ.get("PBR_HIP_LIB"):          # an alternative build of the same source (scripts/lab.sh)
        hip = ctypes.CDLL(os.environ["PBR_HIP_LIB"], mode=ctypes.RTLD_GLOBAL)
    elif _lab and os.environ.get("PBR_GUARD") == "1":   # every device loop bounded (build.py)
        hip = _load(_build.HIP_GUARD_LIB, lambda force=False: _build.build_hip(force, guard=True))
    else:
        hip = _load(_build.HIP_LIB, _build.build_hip)
    host = _load(_build.HOST_LIB, _build.build_host)
except Exception as exc:  # no fallback by design
    raise ImportError("the HIP core (csrc/libpbrhip.so) / host library could not be loaded or built: %s" % exc)

_fp = ctypes.POINTER(ctypes.c_float)
_vp = ctypes.c_void_p

# the struct mirrors below are written against this version of include/pbr_hip.h (pbr_config: 68 bytes since version 5).
# A library of another ABI version must not be handed them; lab runs that load an older build on purpose (PBR_HIP_LIB) say so.
ABI_VERSION = 19
if hasattr(hip, "pbr_abi_version"):
    hip.pbr_abi_version.restype = ctypes.c_uint32
    if hip.pbr_abi_version() != ABI_VERSION and not _lab:
        raise ImportError("libpbrhip.so speaks ABI version %d, this harness %d (include/pbr_hip.h, PBR_ABI_VERSION)" % (hip.pbr_abi_version(), ABI_VERSION))
elif not _lab:
    raise ImportError("libpbrhip.so has no pbr_abi_version(): a build older than round 6")

hip.pbr_create.argtypes = [ctypes.c_int, ctypes.POINTER(_vp)]
hip.pbr_destroy.argtypes = [_vp]
hip.pbr_destroy.restype = None
hip.pbr_last_error.argtypes = [_vp]
hip.pbr_last_error.restype = ctypes.c_char_p
hip.pbr_upload_scene.argtypes = [_vp, ctypes.POINTER(SceneDesc)]
hip.pbr_configure.argtypes = [_vp, ctypes.POINTER(Config)]
hip.pbr_validate_scene.argtypes = [ctypes.POINTER(SceneDesc), ctypes.c_char_p, ctypes.c_size_t]
hip.pbr_write_input.argtypes = [_vp, _fp]
hip.pbr_reset_accum.argtypes = [_vp]
hip.pbr_render_frame.argtypes = [_vp, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.POINTER(Camera)]
hip.pbr_accumulate.argtypes = [_vp]
hip.pbr_render.argtypes = [_vp, ctypes.c_uint32, ctypes.c_uint32, _fp, ctypes.c_float, ctypes.POINTER(Camera)]
hip.pbr_read_output.argtypes = [_vp, _fp]
hip.pbr_read_debug.argtypes = [_vp, _fp]
hip.pbr_read_display.argtypes = [_vp, ctypes.c_void_p, ctypes.c_int]
hip.pbr_denoise.argtypes = [_vp, ctypes.c_float, ctypes.POINTER(Camera), ctypes.POINTER(DenoiseParams), _fp, _fp]
hip.pbr_bvh_node_capacity.argtypes = [ctypes.c_uint32]
hip.pbr_bvh_node_capacity.restype = ctypes.c_uint32
hip.pbr_build_bvh.argtypes = [_vp, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p, ctypes.c_void_p]
hip.pbr_get_focus_depth.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]
hip.pbr_set_focus_depth.argtypes = [_vp, ctypes.c_float]
hip.pbr_read_full.argtypes = [_vp, _fp]
hip.pbr_get_counters.argtypes = [_vp, ctypes.POINTER(Counters)]
hip.pbr_last_kernel_ms.argtypes = [_vp]
hip.pbr_last_kernel_ms.restype = ctypes.c_double
hip.pbr_tile_bytes.argtypes = [_vp]
hip.pbr_tile_bytes.restype = ctypes.c_uint64
hip.pbr_export_tiles.argtypes = [_vp, _vp]
hip.pbr_import_tiles.argtypes = [_vp, _vp]
_ip = ctypes.POINTER(ctypes.c_int32)
_up = ctypes.POINTER(ctypes.c_uint32)
hip.pbr_diag_math.argtypes = [_vp, ctypes.c_int, _fp, _fp, ctypes.c_int, _fp]
hip.pbr_diag_trace.argtypes = [_vp, _fp, ctypes.c_int, _fp, _ip, _fp, _up]
hip.pbr_diag_brdf.argtypes = [_vp, _fp, ctypes.c_int, _fp]
hip.pbr_diag_new_ray.argtypes = [_vp, _fp, ctypes.c_int, _fp]
hip.pbr_diag_guard_trips.argtypes = [_vp, _up]
hip.pbr_diag_last_trace.argtypes = [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)]
hip.pbr_diag_last_plan.argtypes = [_vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
hip.pbr_diag_pin_plan.argtypes = [_vp, ctypes.c_int]
# entry points that older builds of the library lack are bound only when they are there: lab runs load other builds of the
# library for A/B comparisons (PBR_HIP_LIB), and a missing symbol must fail where it is called, not at import
for _name, _args in (
        ("pbr_diag_scene_bytes", [_vp, ctypes.POINTER(ctypes.c_uint64)]),
        ("pbr_mode_built", [ctypes.c_uint32, ctypes.c_uint32]),
        ("pbr_diag_last_kernel", [_vp, ctypes.c_char_p, ctypes.c_size_t]),
        ("pbr_diag_launch_fit", [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
        ("pbr_diag_set_knob", [_vp, ctypes.c_char_p, ctypes.c_int]),                 # absent from round 2's library
        ("pbr_diag_get_tile_order", [_vp, ctypes.c_int, _up, ctypes.c_uint32, _up, _up]),          # round 6
        ("pbr_diag_set_tile_order", [_vp, _up, ctypes.c_uint32, _up]),
        ("pbr_diag_last_deal", [_vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]),
        ("pbr_diag_bvh_build_info", [_vp, ctypes.POINTER(ctypes.c_int)]),
        ("pbr_render_dof", [_vp, ctypes.c_uint32, ctypes.c_uint32, _fp, ctypes.c_float, ctypes.POINTER(Camera)]),       # ABI version 7
        ("pbr_diag_last_focus_chain", [_vp, ctypes.POINTER(ctypes.c_double)]),
        ("pbr_render_adaptive", [_vp, ctypes.c_uint32, _fp, ctypes.c_float, ctypes.POINTER(Camera), ctypes.POINTER(AdaptiveParams)]),   # ABI version 8
        ("pbr_read_tile_stats", [_vp, _up, _fp, ctypes.c_uint32, _up]),
        ("pbr_diag_last_adaptive", [_vp, _up, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]),
        ("pbr_update_vertices", [_vp, ctypes.c_void_p, ctypes.c_uint32]),                                                # ABI version 9
        ("pbr_read_bvh", [_vp, ctypes.c_void_p, ctypes.c_uint32, _up]),
        ("pbr_diag_refit_info", [_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.c_size_t]),
        ("pbr_read_variance", [_vp, _fp]),                                                                               # ABI version 10
        ("pbr_denoise_guided", [_vp, ctypes.c_float, ctypes.POINTER(Camera), ctypes.POINTER(GuidedDenoiseParams), _fp, _fp, _fp]),
        ("pbr_temporal_reset", [_vp]),                                                                                   # ABI version 11
        ("pbr_denoise_temporal", [_vp, ctypes.c_float, ctypes.POINTER(Camera), ctypes.POINTER(TemporalParams), ctypes.POINTER(GuidedDenoiseParams),
                                  _fp, _fp, _fp, _fp]),
        ("pbr_temporal_track_motion", [_vp, ctypes.c_int]),                                                              # ABI version 12
        ("pbr_read_temporal_motion", [_vp, _fp, ctypes.POINTER(ctypes.c_int32)]),
        ("pbr_refit_ordered_walk", [_vp, ctypes.c_int]),                                                                 # ABI version 13
        ("pbr_diag_read_walk", [_vp, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int), _up]),
        ("pbr_diag_relink_info", [_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]),
        ("pbr_update_geometry", [_vp, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]),             # ABI version 14
        ("pbr_diag_patch_refit_info", [_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_float)]),
        ("pbr_diag_read_patches", [_vp, ctypes.c_void_p, ctypes.c_uint32, _up]),
        ("pbr_set_parts", [_vp, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]),      # ABI version 15
        ("pbr_update_transforms", [_vp, ctypes.c_void_p, ctypes.c_uint32]),
        ("pbr_read_geometry", [_vp, ctypes.c_void_p, ctypes.c_uint32, _up, ctypes.c_void_p, ctypes.c_uint32, _up]),
        ("pbr_diag_transform_info", [_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]),
        ("pbr_set_skin", [_vp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]),  # ABI version 16
        ("pbr_update_skin", [_vp, ctypes.c_void_p, ctypes.c_uint32]),
        ("pbr_diag_skin_info", [_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]),
        ("pbr_set_morph", [_vp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),  # ABI version 17
        ("pbr_update_morph", [_vp, ctypes.c_void_p, ctypes.c_uint32]),
        ("pbr_update_pose", [_vp, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]),
        ("pbr_diag_morph_info", [_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]),
        ("pbr_update_skin_dq", [_vp, ctypes.c_void_p, ctypes.c_uint32]),                                                # ABI version 18
        ("pbr_update_pose_dq", [_vp, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]),
        ("pbr_dual_quats_from_matrices", [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]),
        ("pbr_diag_skin_dq_info", [_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]),
        ("pbr_display", [_vp, ctypes.POINTER(DisplayParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(DisplayInfo)]),   # ABI version 19
        ("pbr_display_reset", [_vp]),
        ("pbr_diag_display_info", [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
        ("pbr_diag_solve_cubic", [_vp, _fp, ctypes.c_int, _fp]),
        ("pbr_diag_phong_face", [_vp, _fp, ctypes.c_int, _fp]),
        ("pbr_diag_camera_ray", [_vp, ctypes.c_float, ctypes.POINTER(Camera), _fp, ctypes.c_int, _fp]),
        ("pbr_diag_intersect", [_vp, ctypes.c_int, _fp, ctypes.c_int, _fp]),
        ("pbr_diag_surface_step", [_vp, _fp, ctypes.c_int, _fp]),
        ("pbr_diag_trace_walk", [_vp, ctypes.c_int, ctypes.c_int, _fp, ctypes.c_uint32, _fp, _ip, _fp, _up]),
        ("pbr_diag_trace_walk_slots", [_vp, ctypes.c_int, _up, _up]),
        ("pbr_diag_filter", [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, _fp, _fp, _fp, _fp, _fp]),
        ("pbr_diag_temporal", [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.POINTER(Camera), ctypes.POINTER(TemporalParams), _fp, _fp, _fp,
                               _fp, _fp, _up, ctypes.POINTER(Camera), ctypes.c_float,
                               ctypes.POINTER(ctypes.c_int32), _up, ctypes.c_uint32, _fp, _fp, ctypes.c_uint32,
                               _fp, _fp, _up, _fp, _fp])):
    if hasattr(hip, _name):
        getattr(hip, _name).argtypes = _args
hip.pbr_diag_tune_budget.argtypes = [_vp, ctypes.POINTER(ctypes.c_uint32)]

host.pbrh_last_error.restype = ctypes.c_char_p
host.pbrh_cfg_set.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
host.pbrh_cfg_get.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
host.pbrh_cfg_load.argtypes = [ctypes.c_char_p]
host.pbrh_scene_load_obj.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
host.pbrh_scene_load_obj.restype = _vp
host.pbrh_scene_generate.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32]
host.pbrh_scene_generate.restype = _vp
host.pbrh_scene_destroy.argtypes = [_vp]
host.pbrh_scene_destroy.restype = None
host.pbrh_scene_desc.argtypes = [_vp, ctypes.POINTER(SceneDesc)]
host.pbrh_scene_info.argtypes = [_vp, ctypes.POINTER(ctypes.c_uint32)]
host.pbrh_scene_config.argtypes = [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(Config)]
host.pbrh_scene_camera.argtypes = [_vp, ctypes.POINTER(Camera)]
host.pbrh_camera_lookat.argtypes = [_fp, _fp, ctypes.POINTER(Camera)]
host.pbrh_pixel_dimension.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float]
host.pbrh_pixel_dimension.restype = ctypes.c_float
host.pbrh_pt_create.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
host.pbrh_pt_create.restype = _vp
host.pbrh_pt_destroy.argtypes = [_vp]
host.pbrh_pt_destroy.restype = None
host.pbrh_pt_init.argtypes = [_vp, _vp, ctypes.c_uint32, ctypes.c_uint32]
host.pbrh_pt_generate_image.argtypes = [_vp, _fp, _fp]
host.pbrh_pt_generate_images.argtypes = [_vp, ctypes.c_uint32, _fp]
if hasattr(host, "pbrh_pt_generate_images_adaptive"):
    host.pbrh_pt_generate_images_adaptive.argtypes = [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, _fp]
if hasattr(host, "pbrh_pt_update_vertices"):
    host.pbrh_pt_update_vertices.argtypes = [_vp, _fp, ctypes.c_uint32]
if hasattr(host, "pbrh_pt_refit_ordered_walk"):
    host.pbrh_pt_refit_ordered_walk.argtypes = [_vp, ctypes.c_int]
if hasattr(host, "pbrh_pt_update_geometry"):
    host.pbrh_pt_update_geometry.argtypes = [_vp, _fp, ctypes.c_uint32, _fp, ctypes.c_uint32]
if hasattr(host, "pbrh_pt_set_parts"):
    host.pbrh_pt_set_parts.argtypes = [_vp, _up, ctypes.c_uint32, _up, ctypes.c_uint32, ctypes.c_uint32]
if hasattr(host, "pbrh_pt_update_transforms"):
    host.pbrh_pt_update_transforms.argtypes = [_vp, _fp, ctypes.c_uint32]
if hasattr(host, "pbrh_pt_set_skin"):
    host.pbrh_pt_set_skin.argtypes = [_vp, _up, _fp, ctypes.c_uint32, _up, _fp, ctypes.c_uint32, ctypes.c_uint32]
if hasattr(host, "pbrh_pt_update_skin"):
    host.pbrh_pt_update_skin.argtypes = [_vp, _fp, ctypes.c_uint32]
if hasattr(host, "pbrh_pt_set_morph"):
    host.pbrh_pt_set_morph.argtypes = [_vp, _up, _up, _fp, _up, _up, _fp, ctypes.c_uint32]
if hasattr(host, "pbrh_pt_update_morph"):
    host.pbrh_pt_update_morph.argtypes = [_vp, _fp, ctypes.c_uint32]
if hasattr(host, "pbrh_pt_update_pose"):
    host.pbrh_pt_update_pose.argtypes = [_vp, _fp, ctypes.c_uint32, _fp, ctypes.c_uint32]
if hasattr(host, "pbrh_pt_update_skin_dq"):
    host.pbrh_pt_update_skin_dq.argtypes = [_vp, _fp, ctypes.c_uint32]
if hasattr(host, "pbrh_pt_update_pose_dq"):
    host.pbrh_pt_update_pose_dq.argtypes = [_vp, _fp, ctypes.c_uint32, _fp, ctypes.c_uint32]
host.pbrh_write_ppm.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
host.pbrh_write_pfm.argtypes = [ctypes.c_char_p, _fp, ctypes.c_uint32, ctypes.c_uint32]
host.pbrh_write_png.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
host.pbrh_write_exr.argtypes = [ctypes.c_char_p, _fp, ctypes.c_uint32, ctypes.c_uint32]
host.pbrh_cl_adaptor_render.argtypes = [_vp, ctypes.c_uint32, ctypes.c_float, _fp, _fp]
host.pbrh_cl_adaptor_render_ex.argtypes = [_vp, ctypes.c_uint32, ctypes.c_float, _fp, _fp, ctypes.c_uint32]
host.pbrh_pt_set_focus.argtypes = [_vp, ctypes.c_int, ctypes.c_int]
host.pbrh_pt_reset_sample_count.argtypes = [_vp]
host.pbrh_pt_sample_count.argtypes = [_vp]
host.pbrh_pt_sample_count.restype = ctypes.c_uint32
host.pbrh_pt_context.argtypes = [_vp]
host.pbrh_pt_context.restype = _vp
host.pbrh_pt_camera.argtypes = [_vp, ctypes.POINTER(Camera)]


class PbrError(RuntimeError):
    pass


def _as_fp(a):
    return a.ctypes.data_as(_fp)


def _skin_arrays(bones, weights):
    """A skin's (n, 4) bones as uint32 and weights as float32, contiguous; None stays None."""
    bones = None if bones is None else np.ascontiguousarray(bones, np.uint32).reshape(-1, 4)
    weights = None if weights is None else np.ascontiguousarray(weights, np.float32).reshape(-1, 4)
    return bones, weights


def _morph_lists(targets, what):
    """Morph targets — a sequence of (indices, deltas) pairs, one per target, deltas (n, 3) or (n, 4) — as pbr_set_morph's
    target-major lists: first (targets + 1, uint32), index (uint32) and delta (entries, 4) float32 with w = 0."""
    first = np.zeros(len(targets) + 1, np.uint32)
    indices, deltas = [], []
    for t, (index, delta) in enumerate(targets):
        index = np.asarray(index, np.uint32).reshape(-1)
        delta = np.asarray(delta, np.float32)
        delta = delta.reshape(index.shape[0], delta.shape[-1] if delta.ndim > 1 else 3)
        if delta.shape[1] not in (3, 4):
            raise ValueError("%s target %d: deltas must be (n, 3) or (n, 4)" % (what, t))
        quad = np.zeros((index.shape[0], 4), np.float32)
        quad[:, :delta.shape[1]] = delta
        indices.append(index)
        deltas.append(quad)
        first[t + 1] = first[t] + index.shape[0]
    index = np.ascontiguousarray(np.concatenate(indices) if indices else np.zeros(0, np.uint32), np.uint32)
    delta = np.ascontiguousarray(np.concatenate(deltas) if deltas else np.zeros((0, 4), np.float32), np.float32)
    # a list without entries still hands the library a pointer: NULL means "no such lists"
    return first, (index if index.size else np.zeros(1, np.uint32)), (delta if delta.size else np.zeros((1, 4), np.float32))


def dual_quats_from_matrices(matrices):
    """pbr_dual_quats_from_matrices: row-major 3 x 4 matrices, (bones, 12) or (bones, 3, 4), as (bones, 8) float32 dual
    quaternions for Device.update_skin_dq.  Host only.  A matrix that is not finite or whose 3 x 3 block is not a rotation
    (scale, shear, a mirror) raises PbrError with the library's message."""
    matrices = np.ascontiguousarray(matrices, np.float32).reshape(-1, 12)
    out = np.zeros((matrices.shape[0], 8), np.float32)
    why = ctypes.create_string_buffer(512)
    if hip.pbr_dual_quats_from_matrices(matrices.ctypes.data, matrices.shape[0], out.ctypes.data, why, len(why)) != 0:
        raise PbrError(why.value.decode())
    return out


# ----------------------------------------------------------------------------------------------
# Cfg (source/Cfg.h) — keys as in the reference's config.json
# ----------------------------------------------------------------------------------------------

def cfg_reset():
    host.pbrh_cfg_reset()


def cfg_set(**kv):
    """cfg_set(**{"render.max_depth": 4})"""
    for k, v in kv.items():
        if isinstance(v, bool):
            v = "true" if v else "false"
        host.pbrh_cfg_set(k.encode(), str(v).encode())


def cfg_get(key):
    buf = ctypes.create_string_buffer(256)
    host.pbrh_cfg_get(key.encode(), buf, 256)
    return buf.value.decode()


def validate_scene(desc):
    """pbr_validate_scene: the upload's checks without a device.  Returns "" or the reason the scene is rejected."""
    buf = ctypes.create_string_buffer(512)
    status = hip.pbr_validate_scene(ctypes.byref(desc), buf, 512)
    return "" if status == PBR_OK else (buf.value.decode() or "invalid scene")


def pixel_dimension(width, height, fov=45.0):
    return float(host.pbrh_pixel_dimension(width, height, fov))


# ----------------------------------------------------------------------------------------------
# Host scene: loader / generator + BVH + packed buffers (GLWidget::loadModel without GL)
# ----------------------------------------------------------------------------------------------

class HostScene:
    def __init__(self, handle):
        self._h = handle
        if not handle:
            raise PbrError(host.pbrh_last_error().decode())
        self.desc = SceneDesc()
        host.pbrh_scene_desc(self._h, ctypes.byref(self.desc))
        info = (ctypes.c_uint32 * 10)()
        host.pbrh_scene_info(self._h, info)
        keys = ("flat_nodes", "faces", "vertices", "materials", "lights", "tree_nodes", "leaves", "depth", "skipped", "objects")
        self.info = dict(zip(keys, [int(v) for v in info]))

    @classmethod
    def load_obj(cls, directory, filename):
        if not directory.endswith("/"):
            directory += "/"
        return cls(host.pbrh_scene_load_obj(directory.encode(), filename.encode()))

    @classmethod
    def generate(cls, kind, seed=1, triangles=0):
        return cls(host.pbrh_scene_generate(kind.encode(), seed, triangles))

    def close(self):
        if getattr(self, "_h", None):
            host.pbrh_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def render_through_cl_adaptor(self, frames, seed_step=0.0333, refeed_every=0):
        """Drive the `CL` look-alike (host/cl_adaptor.h) the way the reference's PathTracer drives CL, at the
        configured window size (cfg window.width / window.height); returns (image, debug), row 0 = bottom."""
        w, h = int(cfg_get("window.width")), int(cfg_get("window.height"))
        image = np.empty((h, w, 4), np.float32)
        debug = np.empty((h, w, 4), np.float32)
        if host.pbrh_cl_adaptor_render_ex(self._h, frames, seed_step, image.ctypes.data_as(_fp), debug.ctypes.data_as(_fp), refeed_every) != 0:
            raise PbrError(host.pbrh_last_error().decode())
        return image, debug

    def config(self, width, height):
        cfg = Config()
        host.pbrh_scene_config(self._h, width, height, ctypes.byref(cfg))
        return cfg

    def camera(self):
        cam = Camera()
        host.pbrh_scene_camera(self._h, ctypes.byref(cam))
        return cam

    def _array(self, ptr, count, dtype, width):
        if not ptr or count == 0:
            return np.zeros((0, width), dtype)
        n = count * width
        buf = (ctypes.c_uint32 * n).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype).reshape(count, width).copy()

    def arrays(self):
        """Copies of the flat wire-format arrays (for tests)."""
        d = self.desc
        mat_floats = 12 if d.brdf == 0 else 16
        return {
            "bvh": self._array(d.bvh, d.num_nodes, np.float32, 8),
            "facesV": self._array(d.facesV, d.num_faces, np.uint32, 4),
            "facesN": self._array(d.facesN, d.num_faces, np.uint32, 4),
            "normals": self._array(d.normals, d.num_normals, np.float32, 4),
            "vertices": self._array(d.vertices, d.num_vertices, np.float32, 4),
            "materials": self._array(d.materials, d.num_materials, np.float32, mat_floats),
            "lights": self._array(d.lights, max(1, d.num_lights), np.float32, 12),
        }


# ----------------------------------------------------------------------------------------------
# Device context: the C ABI of include/pbr_hip.h
# ----------------------------------------------------------------------------------------------

# Lab scripts and A/B runs steer the library through environment variables; the LIBRARY reads none (include/pbr_hip_diag.h,
# pbr_diag_set_knob) — this harness maps them onto knobs when a context is created, and ONLY when PBR_LAB_ENV=1 says that
# the process is a lab run (round 4: a stray PBR_* variable in a user's environment must not change the schedule of a
# product render; scripts/*.py and scripts/*.sh set PBR_LAB_ENV themselves).
_ENV_KNOBS = {
    "PBR_LDS_SLOTS": "lds_slots", "PBR_BLOCKS_PER_CU": "blocks_per_cu", "PBR_PH_PARK": "ph_park", "PBR_PH_SHADE": "ph_shade",
    "PBR_PARK_EIGHTHS": "park_eighths", "PBR_DRAIN_MODE": "drain_mode", "PBR_REFILL_BATCH": "refill_batch",
    "PBR_CHUNK_FRAMES": "chunk_frames", "PBR_FACE_NORMALS": "face_normals", "PBR_PLOC_RADIUS": "ploc_radius", "PBR_TUNE_LOG": "tune_log",
    "PBR_DEAL_ORDER": "deal_order",
}


class Device:
    def __init__(self, device=0):
        self._ctx = _vp()
        status = hip.pbr_create(device, ctypes.byref(self._ctx))
        if status != PBR_OK:
            msg = hip.pbr_last_error(self._ctx).decode() if self._ctx else "pbr_create failed"
            if self._ctx:
                hip.pbr_destroy(self._ctx)
                self._ctx = None
            raise PbrError(msg)
        self.width = self.height = 0
        self._shard = (1, 0)
        if os.environ.get("PBR_LAB_ENV") == "1":
            self._apply_lab_environment()

    def _apply_lab_environment(self):
        """PBR_* variables -> knobs / pinned plan, for lab scripts (opt-in: PBR_LAB_ENV=1)."""
        if not hasattr(hip, "pbr_diag_set_knob"):
            raise PbrError("PBR_LAB_ENV=1, but this libpbrhip has no pbr_diag_set_knob")
        for var, knob in _ENV_KNOBS.items():
            if os.environ.get(var):
                self.set_knob(knob, int(os.environ[var]))
        builder = os.environ.get("PBR_BVH_BUILDER")
        if builder:
            if builder not in ("ploc", "lbvh"):
                raise PbrError("PBR_BVH_BUILDER must be 'ploc' or 'lbvh', not %r" % builder)
            self.set_knob("bvh_builder", {"ploc": 0, "lbvh": 1}[builder])
        if os.environ.get("PBR_PLAN"):
            self.pin_plan(int(os.environ["PBR_PLAN"]))

    def set_knob(self, name, value):
        """pbr_diag_set_knob: experiment / test knobs of this context (include/pbr_hip_diag.h); -1 = the default."""
        self._check(hip.pbr_diag_set_knob(self._ctx, name.encode(), int(value)))

    def close(self):
        if getattr(self, "_ctx", None):
            hip.pbr_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        self.close()

    def _check(self, status):
        if status != PBR_OK:
            raise PbrError("%d: %s" % (status, hip.pbr_last_error(self._ctx).decode()))

    def upload_scene(self, desc):
        self._check(hip.pbr_upload_scene(self._ctx, ctypes.byref(desc)))

    def update_vertices(self, vertices):
        """pbr_update_vertices: new positions, (n, 4) float32 with n as uploaded, for the uploaded scene; face records, face
        normals and every node's box are rebuilt on the device (a refit: the tree's links stay).  Afterwards every call gives
        bit for bit what it gives after a fresh upload of the scene with these vertices and the nodes read_bvh() returns."""
        vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 4)
        self._check(hip.pbr_update_vertices(self._ctx, vertices.ctypes.data, vertices.shape[0]))

    def update_geometry(self, vertices, normals=None):
        """pbr_update_geometry: new positions (n, 4) and, unless None, new vertex normals (m, 4), float32 with n and m as uploaded.
        What update_vertices rebuilds plus the Phong patch records; the boxes are thick ones for the configured
        phong_tessellation, so it works while Phong tessellation is configured.  normals=None keeps the context's normals."""
        vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 4)
        if normals is None:
            self._check(hip.pbr_update_geometry(self._ctx, vertices.ctypes.data, vertices.shape[0], None, 0))
            return
        normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 4)
        self._check(hip.pbr_update_geometry(self._ctx, vertices.ctypes.data, vertices.shape[0], normals.ctypes.data, normals.shape[0]))

    def set_parts(self, vertex_part, normal_part=None, num_parts=None):
        """pbr_set_parts: the part of every vertex and, unless None, of every vertex normal (uint32, counts as uploaded), and the
        number of parts (default: the largest index + 1).  Captures the rest pose — the positions and normals the context holds
        now.  set_parts(None) drops the parts."""
        if vertex_part is None:
            self._check(hip.pbr_set_parts(self._ctx, None, 0, None, 0, 0))
            return
        vertex_part = np.ascontiguousarray(vertex_part, np.uint32).reshape(-1)
        if normal_part is not None:
            normal_part = np.ascontiguousarray(normal_part, np.uint32).reshape(-1)
        if num_parts is None:
            num_parts = int(max(vertex_part.max(initial=0), 0 if normal_part is None else normal_part.max(initial=0))) + 1
        self._check(hip.pbr_set_parts(self._ctx, vertex_part.ctypes.data, vertex_part.shape[0], None if normal_part is None else normal_part.ctypes.data,
                                      0 if normal_part is None else normal_part.shape[0], num_parts))

    def update_transforms(self, matrices):
        """pbr_update_transforms: one row-major 3 x 4 matrix per part, (parts, 12) or (parts, 3, 4) float32.  Positions and
        normals are computed on the device from the rest pose of set_parts; everything behind is update_geometry's."""
        matrices = np.ascontiguousarray(matrices, np.float32).reshape(-1, 12)
        self._check(hip.pbr_update_transforms(self._ctx, matrices.ctypes.data, matrices.shape[0]))

    def read_geometry(self):
        """pbr_read_geometry: (positions (n, 4), normals (m, 4)) as the context holds them now, float32; m = 0 for a scene
        without usable vertex normals."""
        nv, nn = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(hip.pbr_read_geometry(self._ctx, None, 0, ctypes.byref(nv), None, 0, ctypes.byref(nn)))
        vertices, normals = np.empty((nv.value, 4), np.float32), np.empty((nn.value, 4), np.float32)
        self._check(hip.pbr_read_geometry(self._ctx, vertices.ctypes.data, nv.value, ctypes.byref(nv), normals.ctypes.data, nn.value, ctypes.byref(nn)))
        return vertices, normals

    def transform_info(self):
        """pbr_diag_transform_info: the parts, the device bytes held for them, the update_transforms calls since set_parts, whether
        the last update was one, and the device time of its transform kernels alone."""
        out, ms = (ctypes.c_uint64 * 4)(), ctypes.c_double()
        self._check(hip.pbr_diag_transform_info(self._ctx, out, ctypes.byref(ms)))
        return {"parts": int(out[0]), "device_bytes": int(out[1]), "updates": int(out[2]), "last_update": bool(out[3]), "ms": float(ms.value)}

    def set_skin(self, vertex_bones, vertex_weights=None, normal_bones=None, normal_weights=None, num_bones=None):
        """pbr_set_skin: four bones (uint32) and four weights (float32) for every vertex and, unless None, for every vertex
        normal — (n, 4) arrays, counts as uploaded —, and the number of bones (default: the largest index + 1).  Captures the
        rest pose — the positions and normals the context holds now.  The weights are used as given.  set_skin(None) drops the
        skin."""
        if vertex_bones is None:
            self._check(hip.pbr_set_skin(self._ctx, None, None, 0, None, None, 0, 0))
            return
        vertex_bones, vertex_weights = _skin_arrays(vertex_bones, vertex_weights)
        normal_bones, normal_weights = _skin_arrays(normal_bones, normal_weights)
        if num_bones is None:
            num_bones = int(max(vertex_bones.max(initial=0), 0 if normal_bones is None else normal_bones.max(initial=0))) + 1
        self._check(hip.pbr_set_skin(self._ctx, vertex_bones.ctypes.data, None if vertex_weights is None else vertex_weights.ctypes.data, vertex_bones.shape[0],
                                     None if normal_bones is None else normal_bones.ctypes.data, None if normal_weights is None else normal_weights.ctypes.data,
                                     0 if normal_bones is None else normal_bones.shape[0], num_bones))

    def update_skin(self, matrices):
        """pbr_update_skin: one row-major 3 x 4 matrix per bone, (bones, 12) or (bones, 3, 4) float32.  Positions and normals
        are blended on the device from the rest pose of set_skin; everything behind is update_geometry's."""
        matrices = np.ascontiguousarray(matrices, np.float32).reshape(-1, 12)
        self._check(hip.pbr_update_skin(self._ctx, matrices.ctypes.data, matrices.shape[0]))

    def skin_info(self):
        """pbr_diag_skin_info: the bones, the device bytes held for the skin, the update_skin calls since set_skin, whether the
        last update was one, and the device time of its skin kernels alone."""
        out, ms = (ctypes.c_uint64 * 4)(), ctypes.c_double()
        self._check(hip.pbr_diag_skin_info(self._ctx, out, ctypes.byref(ms)))
        return {"bones": int(out[0]), "device_bytes": int(out[1]), "updates": int(out[2]), "last_update": bool(out[3]), "ms": float(ms.value)}

    def set_morph(self, vertex_targets, normal_targets=None):
        """pbr_set_morph: sparse morph targets, one (indices, deltas) pair per target — indices uint32, deltas (n, 3) or (n, 4)
        float32 — for the vertices and, unless None, as many pairs for the vertex normals.  Captures the rest pose — the
        positions and normals the context holds now.  set_morph(None) drops the morph."""
        if vertex_targets is None:
            self._check(hip.pbr_set_morph(self._ctx, None, None, None, None, None, None, 0))
            return
        if normal_targets is not None and len(normal_targets) != len(vertex_targets):
            raise ValueError("set_morph: %d vertex targets, %d normal targets" % (len(vertex_targets), len(normal_targets)))
        v = _morph_lists(vertex_targets, "vertex")
        n = (None, None, None) if normal_targets is None else _morph_lists(normal_targets, "normal")
        self._check(hip.pbr_set_morph(self._ctx, *[a.ctypes.data for a in v], *[None if a is None else a.ctypes.data for a in n], len(vertex_targets)))

    def update_morph(self, weights):
        """pbr_update_morph: one float32 weight per target, used as given.  Positions and normals are morphed on the device from
        the rest pose of set_morph; everything behind is update_geometry's."""
        weights = np.ascontiguousarray(weights, np.float32).reshape(-1)
        self._check(hip.pbr_update_morph(self._ctx, weights.ctypes.data, weights.shape[0]))

    def update_pose(self, weights, matrices):
        """pbr_update_pose: the skin of the morphed rest pose — update_morph's weights and update_skin's matrices in one call."""
        weights = np.ascontiguousarray(weights, np.float32).reshape(-1)
        matrices = np.ascontiguousarray(matrices, np.float32).reshape(-1, 12)
        self._check(hip.pbr_update_pose(self._ctx, weights.ctypes.data, weights.shape[0], matrices.ctypes.data, matrices.shape[0]))

    def morph_info(self):
        """pbr_diag_morph_info: the targets, the vertex and normal entries, the device bytes held for the morph, the update_morph
        and update_pose calls since set_morph, the last update (0 none of the two, 1 morph, 2 pose), and the device time of its
        morph / pose kernels alone."""
        out, ms = (ctypes.c_uint64 * 6)(), ctypes.c_double()
        self._check(hip.pbr_diag_morph_info(self._ctx, out, ctypes.byref(ms)))
        return {"targets": int(out[0]), "vertex_entries": int(out[1]), "normal_entries": int(out[2]), "device_bytes": int(out[3]),
                "updates": int(out[4]), "last_update": int(out[5]), "ms": float(ms.value)}

    def update_skin_dq(self, dual_quats):
        """pbr_update_skin_dq: one dual quaternion per bone, (bones, 8) float32 { rx, ry, rz, rw, dx, dy, dz, dw } — the rotation
        quaternion, vector part first, and the dual part 1/2 t r (dual_quats_from_matrices makes them).  The influences and the
        rest pose are set_skin's; everything behind is update_geometry's."""
        dual_quats = np.ascontiguousarray(dual_quats, np.float32).reshape(-1, 8)
        self._check(hip.pbr_update_skin_dq(self._ctx, dual_quats.ctypes.data, dual_quats.shape[0]))

    def update_pose_dq(self, weights, dual_quats):
        """pbr_update_pose_dq: the dual-quaternion skin of the morphed rest pose — update_morph's weights and update_skin_dq's
        dual quaternions in one call."""
        weights = np.ascontiguousarray(weights, np.float32).reshape(-1)
        dual_quats = np.ascontiguousarray(dual_quats, np.float32).reshape(-1, 8)
        self._check(hip.pbr_update_pose_dq(self._ctx, weights.ctypes.data, weights.shape[0], dual_quats.ctypes.data, dual_quats.shape[0]))

    def skin_dq_info(self):
        """pbr_diag_skin_dq_info: the update_skin_dq and update_pose_dq calls since set_skin, the last update (0 none of the two,
        1 skin_dq, 2 pose_dq), and the device time of its dq kernels alone."""
        out, ms = (ctypes.c_uint64 * 2)(), ctypes.c_double()
        self._check(hip.pbr_diag_skin_dq_info(self._ctx, out, ctypes.byref(ms)))
        return {"updates": int(out[0]), "last_update": int(out[1]), "ms": float(ms.value)}

    def read_patches(self):
        """pbr_diag_read_patches: the Phong patch records on the device, (faces, 6, 4) float32 — three corners, three normals."""
        n = ctypes.c_uint32()
        self._check(hip.pbr_diag_read_patches(self._ctx, None, 0, ctypes.byref(n)))
        quads = np.empty((n.value // 6, 6, 4), np.float32)
        self._check(hip.pbr_diag_read_patches(self._ctx, quads.ctypes.data, n.value, ctypes.byref(n)))
        return quads

    def patch_refit_info(self):
        """pbr_diag_patch_refit_info: whether the scene has patches, the device bytes update_geometry holds, its calls since the
        upload, whether the last update was one of them and the phong_tessellation it built its boxes with."""
        out, alpha = (ctypes.c_uint64 * 4)(), ctypes.c_float()
        self._check(hip.pbr_diag_patch_refit_info(self._ctx, out, ctypes.byref(alpha)))
        return {"patches": bool(out[0]), "device_bytes": int(out[1]), "updates": int(out[2]), "last_update": bool(out[3]), "alpha": float(alpha.value)}

    def refit_ordered_walk(self, on):
        """pbr_refit_ordered_walk: while on, update_vertices works under a ray-ordered traversal — the configured layout's records
        are rebuilt on the device, byte for byte what configure( traversal 0 ), update, configure( ordered ) leaves."""
        self._check(hip.pbr_refit_ordered_walk(self._ctx, 1 if on else 0))

    def read_walk(self):
        """pbr_diag_read_walk: (the configured ordered layout's device buffer as uint8, header included; first[8]; hot slots)."""
        size, first, hot = ctypes.c_uint64(), (ctypes.c_int * 8)(), ctypes.c_uint32()
        self._check(hip.pbr_diag_read_walk(self._ctx, None, 0, ctypes.byref(size), first, ctypes.byref(hot)))
        data = np.empty(size.value, np.uint8)
        self._check(hip.pbr_diag_read_walk(self._ctx, data.ctypes.data, size.value, ctypes.byref(size), first, ctypes.byref(hot)))
        return data, [int(v) for v in first], int(hot.value)

    def relink_info(self):
        """pbr_diag_relink_info: the re-link's table bytes, levels, the last update's launches and whether it re-linked, its ms."""
        out, ms = (ctypes.c_uint64 * 4)(), ctypes.c_double()
        self._check(hip.pbr_diag_relink_info(self._ctx, out, ctypes.byref(ms)))
        return {"table_bytes": int(out[0]), "levels": int(out[1]), "launches": int(out[2]), "relinked": bool(out[3]), "ms": float(ms.value)}

    def read_bvh(self):
        """pbr_read_bvh: the current tree, (nodes, 8) float32 in the wire format — the uploaded nodes, after update_vertices
        with the refitted boxes."""
        n = ctypes.c_uint32()
        self._check(hip.pbr_read_bvh(self._ctx, None, 0, ctypes.byref(n)))
        nodes = np.empty((n.value, 8), np.float32)
        self._check(hip.pbr_read_bvh(self._ctx, nodes.ctypes.data, n.value, ctypes.byref(n)))
        return nodes

    def refit_info(self):
        """pbr_diag_refit_info: what the upload keeps for update_vertices, and the last update's vertex copy time."""
        out, ms, why = (ctypes.c_uint64 * 8)(), ctypes.c_double(), ctypes.create_string_buffer(256)
        self._check(hip.pbr_diag_refit_info(self._ctx, out, ctypes.byref(ms), why, 256))
        keys = ("nested", "subtree_cap", "workgroups", "subtrees", "top_nodes", "top_levels", "device_bytes", "updates")
        info = dict(zip(keys, [int(v) for v in out]))
        info["nested"], info["upload_ms"], info["why"] = bool(info["nested"]), float(ms.value), why.value.decode()
        return info

    def configure(self, cfg):
        self._check(hip.pbr_configure(self._ctx, ctypes.byref(cfg)))
        self.width, self.height = int(cfg.width), int(cfg.height)
        self._shard = (int(cfg.tile_world), int(cfg.tile_rank))

    def write_input(self, rgba):
        rgba = np.ascontiguousarray(rgba, np.float32)
        assert rgba.size == self.width * self.height * 4
        self._check(hip.pbr_write_input(self._ctx, _as_fp(rgba)))

    def reset_accum(self):
        self._check(hip.pbr_reset_accum(self._ctx))

    def render_frame(self, seed, pixel_weight, px_dim, cam):
        self._check(hip.pbr_render_frame(self._ctx, seed, pixel_weight, px_dim, ctypes.byref(cam)))

    def accumulate(self):
        self._check(hip.pbr_accumulate(self._ctx))

    def render(self, first_sample_count, seeds, px_dim, cam):
        seeds = np.ascontiguousarray(seeds, np.float32)
        self._check(hip.pbr_render(self._ctx, first_sample_count, len(seeds), _as_fp(seeds), px_dim, ctypes.byref(cam)))

    def render_dof(self, first_sample_count, seeds, px_dim, cam):
        """pbr_render_dof: `render` for a camera with a focus point — the frames of a depth-of-field render in one call, bit-identical
        to render_frame + accumulate per frame.  With tile sharding: one set_focus_depth before the call."""
        seeds = np.ascontiguousarray(seeds, np.float32)
        self._check(hip.pbr_render_dof(self._ctx, first_sample_count, len(seeds), _as_fp(seeds), px_dim, ctypes.byref(cam)))

    def render_adaptive(self, first_sample_count, seeds, px_dim, cam, min_frames, round_frames, max_frames, threshold):
        """pbr_render_adaptive: `render` in rounds — min_frames for every tile, then round_frames at a time for the tiles whose
        error estimate (the relative standard error of the tile's mean luminance) is still above `threshold`, max_frames =
        len(seeds) at most.  A tile that stopped after c frames holds what render(first_sample_count, seeds[:c]) leaves there."""
        seeds = np.ascontiguousarray(seeds, np.float32)
        if len(seeds) != max_frames:
            raise PbrError("render_adaptive: %d seeds for max_frames = %d" % (len(seeds), max_frames))
        params = AdaptiveParams(min_frames, round_frames, max_frames, threshold)
        self._check(hip.pbr_render_adaptive(self._ctx, first_sample_count, _as_fp(seeds), px_dim, ctypes.byref(cam), ctypes.byref(params)))

    def tile_stats(self):
        """pbr_read_tile_stats: (frames, error) of the last render_adaptive per tile — frames rendered, and the error estimate
        at the tile's last test.  Unsharded context: two (tiles_y, tiles_x) arrays, row 0 = the bottom tile row like
        read_output.  A shard (tile_world > 1): (frames, error, tile_ids) in local-tile order, tile_ids = the tiles' global
        indices ty * tiles_x + tx (tiles.local_tile_ids)."""
        n = ctypes.c_uint32()
        self._check(hip.pbr_read_tile_stats(self._ctx, None, None, 0, ctypes.byref(n)))
        frames, error = np.empty(n.value, np.uint32), np.empty(n.value, np.float32)
        self._check(hip.pbr_read_tile_stats(self._ctx, frames.ctypes.data_as(_up), _as_fp(error), n.value, ctypes.byref(n)))
        world, rank = self._shard
        if world <= 1:
            shape = (self.height // tiles.TILE, self.width // tiles.TILE)
            return frames.reshape(shape), error.reshape(shape)
        return frames, error, tiles.local_tile_ids(self.width, self.height, world, rank)

    def last_adaptive(self):
        """pbr_diag_last_adaptive: (rounds, (pixel, frame) units traced, ms inside the folds) of the last render_adaptive."""
        rounds, units, ms = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_double()
        self._check(hip.pbr_diag_last_adaptive(self._ctx, ctypes.byref(rounds), ctypes.byref(units), ctypes.byref(ms)))
        return int(rounds.value), int(units.value), float(ms.value)

    def _read(self, fn):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(fn(self._ctx, _as_fp(out)))
        return out

    def read_output(self):
        return self._read(hip.pbr_read_output)

    def read_debug(self):
        return self._read(hip.pbr_read_debug)

    def read_full(self):
        return self._read(hip.pbr_read_full)

    def build_bvh(self, vertices, facesV, facesN):
        """pbr_build_bvh: BVH built on the device (Morton order + clustering by surface area).  vertices (n, 4) float32, facesV / facesN (m, 4) uint32 ->
        (nodes (k, 8) float32 in the reference's flat format, facesV and facesN in leaf order)."""
        vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 4)
        facesV = np.ascontiguousarray(facesV, np.uint32).reshape(-1, 4)
        facesN = np.ascontiguousarray(facesN, np.uint32).reshape(-1, 4)
        m = facesV.shape[0]
        nodes = np.zeros((int(hip.pbr_bvh_node_capacity(m)), 8), np.float32)
        outV, outN = np.empty_like(facesV), np.empty_like(facesN)
        count = ctypes.c_uint32()
        self._check(hip.pbr_build_bvh(self._ctx, vertices.ctypes.data, vertices.shape[0], facesV.ctypes.data, facesN.ctypes.data, m,
                                      nodes.ctypes.data, ctypes.byref(count), outV.ctypes.data, outN.ctypes.data))
        return nodes[:count.value].copy(), outV, outN

    def get_focus_depth(self, x, y):
        """(previous-frame distance of pixel (x, y), whether this rank owns its tile) — DOF with tile sharding."""
        t, owned = ctypes.c_float(), ctypes.c_int()
        self._check(hip.pbr_get_focus_depth(self._ctx, x, y, ctypes.byref(t), ctypes.byref(owned)))
        return float(t.value), bool(owned.value)

    def set_focus_depth(self, t):
        self._check(hip.pbr_set_focus_depth(self._ctx, t))

    def read_display(self, top_row_first=False):
        """imageOut as (H, W, 4) uint8 — what the reference's GL viewer shows (clamped linear colour)."""
        out = np.empty((self.height, self.width, 4), np.uint8)
        self._check(hip.pbr_read_display(self._ctx, out.ctypes.data, 1 if top_row_first else 0))
        return out

    def display(self, params=None, rgba=None, top_row_first=False, info=False):
        """pbr_display: the accumulated image — or `rgba`, an (H, W, 4) float32 image with row 0 at the bottom, as read_output,
        read_full and the denoise calls return it — through exposure, tone curve and transfer function (DisplayParams) to
        (H, W, 4) uint8.  With info=True also a dict: exposure, log2_target, log2_used, counted, dark, histogram (256 uint32)."""
        params = params if params is not None else DisplayParams()
        out = np.empty((self.height, self.width, 4), np.uint8)
        if rgba is not None:
            rgba = np.ascontiguousarray(rgba, np.float32)
            if rgba.shape != (self.height, self.width, 4):
                raise PbrError("display: rgba is %r, the configured image (%d, %d, 4)" % (rgba.shape, self.height, self.width))
        record = DisplayInfo() if info else None
        self._check(hip.pbr_display(self._ctx, ctypes.byref(params), None if rgba is None else rgba.ctypes.data, out.ctypes.data,
                                    1 if top_row_first else 0, ctypes.byref(record) if info else None))
        if not info:
            return out
        return out, {"exposure": float(record.exposure), "log2_target": float(record.log2_target), "log2_used": float(record.log2_used),
                     "counted": int(record.counted), "dark": int(record.dark), "histogram": np.array(record.histogram, np.uint32)}

    def display_reset(self):
        """pbr_display_reset: forgets the adapted exposure; the next auto display jumps to its target."""
        self._check(hip.pbr_display_reset(self._ctx))

    def display_info(self):
        """pbr_diag_display_info: (histogram kernel ms, map kernel ms) of the last display."""
        hist, mapped = ctypes.c_double(), ctypes.c_double()
        self._check(hip.pbr_diag_display_info(self._ctx, ctypes.byref(hist), ctypes.byref(mapped)))
        return float(hist.value), float(mapped.value)

    def denoise(self, px_dim, cam, params=None, features=False):
        """pbr_denoise: the accumulated image after the edge-avoiding a-trous filter, (H, W, 4) float32 (the accumulation
        is not modified); with features=True also the first-hit feature buffers (3, H, W, 4): position | t, normal | hit,
        Kd | material."""
        params = params if params is not None else DenoiseParams()
        out = np.empty((self.height, self.width, 4), np.float32)
        feat = np.empty((3, self.height, self.width, 4), np.float32) if features else None
        self._check(hip.pbr_denoise(self._ctx, px_dim, ctypes.byref(cam), ctypes.byref(params), out.ctypes.data_as(_fp),
                                    feat.ctypes.data_as(_fp) if features else None))
        return (out, feat) if features else out

    def read_variance(self):
        """pbr_read_variance: (H, W) float32, the variance of every pixel's mean luminance as the last render_adaptive
        estimated it (M2 / (c - 1) / (first_sample_count + c), c the frames of the pixel's tile)."""
        out = np.empty((self.height, self.width), np.float32)
        self._check(hip.pbr_read_variance(self._ctx, _as_fp(out)))
        return out

    def denoise_guided(self, px_dim, cam, params=None, variance=False, features=False):
        """pbr_denoise_guided: `denoise` right behind render_adaptive, with a luminance term in units of the local standard
        deviation in place of sigma_color.  (H, W, 4) float32; with variance=True also the filtered variance (H, W), with
        features=True the feature buffers as `denoise` gives them — in that order."""
        params = params if params is not None else GuidedDenoiseParams()
        out = np.empty((self.height, self.width, 4), np.float32)
        var = np.empty((self.height, self.width), np.float32) if variance else None
        feat = np.empty((3, self.height, self.width, 4), np.float32) if features else None
        self._check(hip.pbr_denoise_guided(self._ctx, px_dim, ctypes.byref(cam), ctypes.byref(params), out.ctypes.data_as(_fp),
                                           var.ctypes.data_as(_fp) if variance else None, feat.ctypes.data_as(_fp) if features else None))
        extra = ([var] if variance else []) + ([feat] if features else [])
        return (out, *extra) if extra else out

    def temporal_reset(self):
        """pbr_temporal_reset: drops denoise_temporal's history; the next call starts at L = 1 everywhere."""
        self._check(hip.pbr_temporal_reset(self._ctx))

    def temporal_track_motion(self, on):
        """pbr_temporal_track_motion: while on, update_vertices keeps denoise_temporal's history, and a call behind an update
        follows every hit pixel's face back to where it was (per-vertex motion).  Off by default; survives configure and
        upload_scene."""
        self._check(hip.pbr_temporal_track_motion(self._ctx, 1 if on else 0))

    def temporal_motion(self):
        """pbr_read_temporal_motion: (motion (H, W, 4) float32 {Pprev, code}, face (H, W) int32, -1 = miss) of the last
        denoise_temporal, if it took the motion path (PbrError otherwise)."""
        motion = np.empty((self.height, self.width, 4), np.float32)
        face = np.empty((self.height, self.width), np.int32)
        self._check(hip.pbr_read_temporal_motion(self._ctx, motion.ctypes.data_as(_fp), face.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return motion, face

    def denoise_temporal(self, px_dim, cam, temporal=None, filter=None, variance=False, integrated=False, history=False):
        """pbr_denoise_temporal: `denoise_guided` with a per-pixel history that is re-projected through the previous call's
        camera — once per render_adaptive, after a camera move too.  (H, W, 4) float32; with variance=True also the filtered
        variance (H, W), with integrated=True the filter's input (H, W, 4) {colour, variance}, with history=True (H, W, 4)
        {fx, fy, L, valid} — in that order."""
        temporal = temporal if temporal is not None else TemporalParams()
        filter = filter if filter is not None else GuidedDenoiseParams()
        out = np.empty((self.height, self.width, 4), np.float32)
        var = np.empty((self.height, self.width), np.float32) if variance else None
        integ = np.empty((self.height, self.width, 4), np.float32) if integrated else None
        hist = np.empty((self.height, self.width, 4), np.float32) if history else None
        self._check(hip.pbr_denoise_temporal(self._ctx, px_dim, ctypes.byref(cam), ctypes.byref(temporal), ctypes.byref(filter),
                                             out.ctypes.data_as(_fp), var.ctypes.data_as(_fp) if variance else None,
                                             integ.ctypes.data_as(_fp) if integrated else None, hist.ctypes.data_as(_fp) if history else None))
        extra = ([var] if variance else []) + ([integ] if integrated else []) + ([hist] if history else [])
        return (out, *extra) if extra else out

    def counters(self):
        c = Counters()
        self._check(hip.pbr_get_counters(self._ctx, ctypes.byref(c)))
        return {"nodes": int(c.nodes), "tris": int(c.tris), "hits": int(c.hits), "paths": int(c.paths)}

    def last_kernel_ms(self):
        return float(hip.pbr_last_kernel_ms(self._ctx))

    def tile_bytes(self):
        return int(hip.pbr_tile_bytes(self._ctx))

    # ---- diagnostic stages (include/pbr_hip_diag.h) ----

    MATH_OPS = {"sin": 0, "cos": 1, "tan": 2, "acos": 3, "atan": 4, "pow": 5, "randhash": 6, "cbrt": 7}

    def diag_math(self, op, x, y=None):
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(x if y is None else y, np.float32)
        out = np.empty_like(x)
        self._check(hip.pbr_diag_math(self._ctx, self.MATH_OPS[op], _as_fp(x), _as_fp(y), x.size, _as_fp(out)))
        return out

    def diag_trace(self, rays):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        t = np.empty(n, np.float32)
        face = np.empty(n, np.int32)
        normal = np.empty((n, 3), np.float32)
        counts = np.empty((n, 2), np.uint32)
        self._check(hip.pbr_diag_trace(self._ctx, _as_fp(rays), n, _as_fp(t), face.ctypes.data_as(_ip),
                                       _as_fp(normal), counts.ctypes.data_as(_up)))
        return t, face, normal, counts

    def diag_trace_walk(self, rays, t0=None, anyhit=False, lds_slots=0):
        """pbr_diag_trace_walk: ray i on thread i of one launch through the walk of the configured traversal AND arithmetic as
        the lock-step render kernels run it — the closest-hit walk, or with anyhit the shadow walk — behind lds_slots staged
        slots.  rays: n x 6 {origin, dir}; t0: what hit.t starts from, per ray or one value (default +inf; the light's
        distance for the shadow walk).  Returns (t, face, normal, counts) as diag_trace."""
        rays = np.asarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        rays8 = np.zeros((n, 8), np.float32)
        rays8[:, 0:3], rays8[:, 4:7] = rays[:, 0:3], rays[:, 3:6]
        rays8[:, 3] = np.inf if t0 is None else np.asarray(t0, np.float32)
        t = np.empty(n, np.float32)
        face = np.empty(n, np.int32)
        normal = np.empty((n, 3), np.float32)
        counts = np.empty((n, 2), np.uint32)
        self._check(hip.pbr_diag_trace_walk(self._ctx, 1 if anyhit else 0, int(lds_slots), _as_fp(rays8), n, _as_fp(t),
                                            face.ctypes.data_as(_ip), _as_fp(normal), counts.ctypes.data_as(_up)))
        return t, face, normal, counts

    def diag_trace_walk_slots(self, lds_slots):
        """pbr_diag_trace_walk_slots: (the slots diag_trace_walk stages for this request, the ranked prefix that bounds them)."""
        slots, hot = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(hip.pbr_diag_trace_walk_slots(self._ctx, int(lds_slots), ctypes.byref(slots), ctypes.byref(hot)))
        return int(slots.value), int(hot.value)

    def diag_brdf(self, items):
        items = np.ascontiguousarray(items, np.float32).reshape(-1, 16)
        out = np.empty((items.shape[0], 4), np.float32)
        self._check(hip.pbr_diag_brdf(self._ctx, _as_fp(items), items.shape[0], _as_fp(out)))
        return out

    def diag_new_ray(self, items):
        items = np.ascontiguousarray(items, np.float32).reshape(-1, 12)
        out = np.empty((items.shape[0], 8), np.float32)
        self._check(hip.pbr_diag_new_ray(self._ctx, _as_fp(items), items.shape[0], _as_fp(out)))
        return out

    def diag_solve_cubic(self, items):
        """pbr_diag_solve_cubic: n x 4 {a0, a1, a2, a3} -> n x 4 {count, x0, x1, x2}."""
        items = np.ascontiguousarray(items, np.float32).reshape(-1, 4)
        out = np.empty((items.shape[0], 4), np.float32)
        self._check(hip.pbr_diag_solve_cubic(self._ctx, _as_fp(items), items.shape[0], _as_fp(out)))
        return out

    def diag_phong_face(self, items):
        """pbr_diag_phong_face: n x 32 {P1, P2, P3, N1, N2, N3, origin, dir, rayT, tNear, tFar, alpha, pad[4]} -> n x 4 {t, normal}."""
        items = np.ascontiguousarray(items, np.float32).reshape(-1, 32)
        out = np.empty((items.shape[0], 4), np.float32)
        self._check(hip.pbr_diag_phong_face(self._ctx, _as_fp(items), items.shape[0], _as_fp(out)))
        return out

    def diag_camera_ray(self, px_dim, cam, items):
        """pbr_diag_camera_ray: n x 8 {px, py, seed, tFocus, tObject, pad[3]} -> n x 8 {origin, dir, seed after, 0}."""
        items = np.ascontiguousarray(items, np.float32).reshape(-1, 8)
        out = np.empty((items.shape[0], 8), np.float32)
        self._check(hip.pbr_diag_camera_ray(self._ctx, px_dim, ctypes.byref(cam), _as_fp(items), items.shape[0], _as_fp(out)))
        return out

    INTERSECT_OPS = {"triangle": 0, "box": 1, "sphere": 2}

    def diag_intersect(self, op, items):
        """pbr_diag_intersect: n x 24 (layout by op, include/pbr_hip_diag.h) -> n x 4."""
        items = np.ascontiguousarray(items, np.float32).reshape(-1, 24)
        out = np.empty((items.shape[0], 4), np.float32)
        self._check(hip.pbr_diag_intersect(self._ctx, self.INTERSECT_OPS[op], _as_fp(items), items.shape[0], _as_fp(out)))
        return out

    def diag_filter(self, kind, image, features, params, px_dim, variance=None):
        """pbr_diag_filter: the a-trous passes of `denoise` (kind 0, params a DenoiseParams) or of `denoise_guided` /
        `denoise_temporal` (kind 1, params a GuidedDenoiseParams, variance (H, W) = V_0) over planes given here: image (H, W, 4),
        features (3, H, W, 4) as `denoise` returns them; any H, W >= 1.  No scene or configuration needed.
        -> rgba (H, W, 4) for kind 0, (rgba, variance (H, W)) for kind 1."""
        image = np.ascontiguousarray(image, np.float32)
        h, w = image.shape[:2]
        features = np.ascontiguousarray(features, np.float32)
        if image.shape != (h, w, 4) or features.shape != (3, h, w, 4):
            raise PbrError("diag_filter: image (H, W, 4) and features (3, H, W, 4)")
        if kind == 1:
            variance = np.ascontiguousarray(variance, np.float32)
            if variance.shape != (h, w):
                raise PbrError("diag_filter: variance (H, W)")
        out = np.empty((h, w, 4), np.float32)
        var = np.empty((h, w), np.float32) if kind == 1 else None
        self._check(hip.pbr_diag_filter(self._ctx, kind, w, h, px_dim, ctypes.addressof(params), _as_fp(image),
                                        _as_fp(variance) if kind == 1 else None, _as_fp(features), _as_fp(out),
                                        _as_fp(var) if kind == 1 else None))
        return (out, var) if kind == 1 else out

    def diag_temporal(self, image, variance, features, cam, px_dim, temporal, prev=None, motion=None, out=None):
        """pbr_diag_temporal: steps 0 to 4 of `denoise_temporal` over planes given here — image (H, W, 4), variance (H, W),
        features (3, H, W, 4) as `denoise` returns them, any H, W >= 1; no scene or configuration needed.  prev: None (no
        history) or a dict integrated (H, W, 4) / features (3, H, W, 4) / lengths (H, W) / cam / px_dim; motion: None or a dict
        face (H, W) int32 / faces_v (faces, 4) uint32 / vertices / hist_vertices (n, 4): the motion path.  out: arrays to write
        into instead of new ones (keys as returned).  -> dict integrated, history (H, W, 4), lengths (H, W) uint32 and, on the
        motion path, motion and reference (H, W, 4).  The library checks the values; this wrapper only the shapes."""
        image, variance = np.ascontiguousarray(image, np.float32), np.ascontiguousarray(variance, np.float32)
        features = np.ascontiguousarray(features, np.float32)
        h, w = variance.shape
        if image.shape != (h, w, 4) or features.shape != (3, h, w, 4):
            raise PbrError("diag_temporal: image (H, W, 4), variance (H, W) and features (3, H, W, 4)")
        keep = []   # the converted inputs must outlive the call

        def held(a, dtype, shape):
            a = np.ascontiguousarray(a, dtype)
            if a.shape != shape:
                raise PbrError("diag_temporal: an input of shape %s where %s is expected" % (a.shape, shape))
            keep.append(a)
            return a

        p_int = p_feat = p_len = p_cam = None
        p_px = 0.0
        if prev is not None:
            p_int = _as_fp(held(prev["integrated"], np.float32, (h, w, 4)))
            p_feat = _as_fp(held(prev["features"], np.float32, (3, h, w, 4)))
            p_len = held(prev["lengths"], np.uint32, (h, w)).ctypes.data_as(_up)
            p_cam, p_px = ctypes.byref(prev["cam"]), prev["px_dim"]
        m_face = m_faces = m_v = m_h = None
        nf = nv = 0
        if motion is not None:
            faces_v = np.ascontiguousarray(motion["faces_v"], np.uint32).reshape(-1, 4)
            vertices = np.ascontiguousarray(motion["vertices"], np.float32).reshape(-1, 4)
            nf, nv = faces_v.shape[0], vertices.shape[0]
            m_face = held(motion["face"], np.int32, (h, w)).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
            m_faces = held(faces_v, np.uint32, (nf, 4)).ctypes.data_as(_up)
            m_v = _as_fp(held(vertices, np.float32, (nv, 4)))
            m_h = _as_fp(held(motion["hist_vertices"], np.float32, (nv, 4)))
        res = dict(out) if out is not None else {}
        for key, dtype, shape in (("integrated", np.float32, (h, w, 4)), ("history", np.float32, (h, w, 4)), ("lengths", np.uint32, (h, w)),
                                  ("motion", np.float32, (h, w, 4)), ("reference", np.float32, (h, w, 4))):
            if key in ("motion", "reference") and motion is None:
                res.pop(key, None)
                continue
            if key not in res:
                res[key] = np.empty(shape, dtype)
            elif res[key].dtype != dtype or res[key].shape != shape or not res[key].flags.c_contiguous:
                raise PbrError("diag_temporal: out[%r] must be a contiguous %s array of shape %s" % (key, np.dtype(dtype).name, shape))
        self._check(hip.pbr_diag_temporal(self._ctx, w, h, px_dim, ctypes.byref(cam), ctypes.byref(temporal), _as_fp(image), _as_fp(variance),
                                          _as_fp(features), p_int, p_feat, p_len, p_cam, p_px, m_face, m_faces, nf, m_v, m_h, nv,
                                          _as_fp(res["integrated"]), _as_fp(res["history"]), res["lengths"].ctypes.data_as(_up),
                                          _as_fp(res["motion"]) if motion is not None else None,
                                          _as_fp(res["reference"]) if motion is not None else None))
        return res

    def diag_surface_step(self, items):
        """pbr_diag_surface_step: n x 24 {origin, dir, normal, t, seed, color, lit, lightDir, lightRgb, pad[3]} -> n x 12
        {newDir, seed after, addDepth, color, finalColor, secondaryPaths increment}."""
        items = np.ascontiguousarray(items, np.float32).reshape(-1, 24)
        out = np.empty((items.shape[0], 12), np.float32)
        self._check(hip.pbr_diag_surface_step(self._ctx, _as_fp(items), items.shape[0], _as_fp(out)))
        return out

    def guard_trips(self):
        out = (ctypes.c_uint32 * 3)()
        self._check(hip.pbr_diag_guard_trips(self._ctx, out))
        return [int(v) for v in out]

    def last_trace(self):
        """(summed duration in ms, number) of the path-tracing launches of the last render."""
        ms, n = ctypes.c_double(), ctypes.c_uint32()
        self._check(hip.pbr_diag_last_trace(self._ctx, ctypes.byref(ms), ctypes.byref(n)))
        return float(ms.value), int(n.value)

    def last_focus_chain_ms(self):
        """Duration in ms of the focus chain (the pre-pass of render_dof) of the last render; 0 for any other render."""
        ms = ctypes.c_double()
        self._check(hip.pbr_diag_last_focus_chain(self._ctx, ctypes.byref(ms)))
        return float(ms.value)

    def last_plan(self):
        """(name of the schedule that rendered the last render, auto-tuner's choice or -1 while measuring)."""
        name, tuned = ctypes.create_string_buffer(48), ctypes.c_int(-1)
        self._check(hip.pbr_diag_last_plan(self._ctx, name, 48, ctypes.byref(tuned)))
        return name.value.decode(), int(tuned.value)

    def scene_bytes(self):
        """Device bytes of the scene: {"nodes": reference-order stream, "walk_streams": the ordered walk's (0 until built), "faces"}."""
        out = (ctypes.c_uint64 * 3)()
        self._check(hip.pbr_diag_scene_bytes(self._ctx, out))
        return {"nodes": int(out[0]), "walk_streams": int(out[1]), "faces": int(out[2])}

    def last_kernel(self):
        """The symbol of the kernel behind last_plan()[0], as a profiler prints it: "ptk_f0::pathTracingDual<1, false, false>"."""
        name = ctypes.create_string_buffer(96)
        self._check(hip.pbr_diag_last_kernel(self._ctx, name, 96))
        return name.value.decode()

    def launch_fit(self):
        """(fixed ms, ms per frame) of a launch of the plan in use, as the schedule tuner fitted them; None without a fit."""
        a, b = ctypes.c_double(), ctypes.c_double()
        if hip.pbr_diag_launch_fit(self._ctx, ctypes.byref(a), ctypes.byref(b)) != PBR_OK:
            return None
        return float(a.value), float(b.value)

    PLAN_NAMES = ("refill-lean", "refill-wide", "phased-lean", "phased-wide", "phased-mid", "refill-mid", "phased-dual")

    def pin_plan(self, plan):
        """Render with schedule `plan` (index into PLAN_NAMES) without tuning; -1 = let the tuner choose."""
        self._check(hip.pbr_diag_pin_plan(self._ctx, int(plan)))

    def tile_order(self, cost_ordered=False, which=None):
        """pbr_diag_get_tile_order: (order, band_first) — the local tiles in the order the queue deals them, band b's
        stretch = order[band_first[b]:band_first[b + 1]]; cost_ordered (which = 1): the library's learnt cost-classes order instead
        of the spatial (or pinned) one; which = 2: its expensive-last order."""
        n, first, which = ctypes.c_uint32(), (ctypes.c_uint32 * 9)(), (which if which is not None else (1 if cost_ordered else 0))
        self._check(hip.pbr_diag_get_tile_order(self._ctx, which, None, 0, ctypes.byref(n), first))
        order = np.empty(n.value, np.uint32)
        self._check(hip.pbr_diag_get_tile_order(self._ctx, which, order.ctypes.data_as(_up), n.value, ctypes.byref(n), first))
        return order, np.array(first[:], np.int64)

    def set_tile_order(self, order, band_first=None):
        """pbr_diag_set_tile_order: deal the tiles in this order until the next pbr_configure — per band a permutation of the
        band's own tiles, or with band_first (9 entries) any partition of the local tiles into eight lists; None hands the order
        back to the library."""
        if order is None:
            self._check(hip.pbr_diag_set_tile_order(self._ctx, None, 0, None))
        else:
            order = np.ascontiguousarray(order, np.uint32)
            first = None if band_first is None else np.ascontiguousarray(band_first, np.uint32)
            self._check(hip.pbr_diag_set_tile_order(self._ctx, order.ctypes.data_as(_up), order.size, None if first is None else first.ctypes.data_as(_up)))

    def bvh_build_radius(self):
        """pbr_diag_bvh_build_info: the clustering radius pbr_build_bvh last used in this context (0: no build yet)."""
        r = ctypes.c_int(0)
        self._check(hip.pbr_diag_bvh_build_info(self._ctx, ctypes.byref(r)))
        return int(r.value)

    def last_deal(self):
        """pbr_diag_last_deal: (the order the last render's largest launch was dealt in, whether a cost order has been learnt)."""
        name, learnt = ctypes.create_string_buffer(16), ctypes.c_int(0)
        self._check(hip.pbr_diag_last_deal(self._ctx, name, 16, ctypes.byref(learnt)))
        return name.value.decode(), bool(learnt.value)

    def tune_budget(self):
        """Frames of the configured size after which the schedule tuner has settled."""
        n = ctypes.c_uint32(0)
        self._check(hip.pbr_diag_tune_budget(self._ctx, ctypes.byref(n)))
        return int(n.value)

    def export_tiles(self, device_ptr):
        self._check(hip.pbr_export_tiles(self._ctx, device_ptr))

    def import_tiles(self, device_ptr):
        self._check(hip.pbr_import_tiles(self._ctx, device_ptr))


def write_ppm(path, rgba8):
    """(H, W, 4) uint8, top row first (Device.read_display(top_row_first=True)) -> binary PPM."""
    rgba8 = np.ascontiguousarray(rgba8, np.uint8)
    if host.pbrh_write_ppm(str(path).encode(), rgba8.ctypes.data, rgba8.shape[1], rgba8.shape[0]) != 0:
        raise PbrError(host.pbrh_last_error().decode())


def write_pfm(path, rgba):
    """(H, W, 4) float32, row 0 = bottom (Device.read_output()) -> PFM, the linear image."""
    rgba = np.ascontiguousarray(rgba, np.float32)
    if host.pbrh_write_pfm(str(path).encode(), _as_fp(rgba), rgba.shape[1], rgba.shape[0]) != 0:
        raise PbrError(host.pbrh_last_error().decode())


def write_png(path, rgba8):
    """(H, W, 4) uint8, top row first (Device.read_display(top_row_first=True)) -> PNG (8-bit RGBA)."""
    rgba8 = np.ascontiguousarray(rgba8, np.uint8)
    if host.pbrh_write_png(str(path).encode(), rgba8.ctypes.data, rgba8.shape[1], rgba8.shape[0]) != 0:
        raise PbrError(host.pbrh_last_error().decode())


def write_exr(path, rgba):
    """(H, W, 4) float32, row 0 = bottom (Device.read_output()) -> OpenEXR: binary32 R, G, B and A = the first-hit distance."""
    rgba = np.ascontiguousarray(rgba, np.float32)
    if host.pbrh_write_exr(str(path).encode(), _as_fp(rgba), rgba.shape[1], rgba.shape[0]) != 0:
        raise PbrError(host.pbrh_last_error().decode())


def frame_seeds(first_sample_count, n_frames, seed_step=0.0333):
    """The fixed seed sequence that stands in for the reference's wall clock
    (PathTracer.cpp:63,78-82): seed_k = step * (k + 1), evaluated in float32."""
    k = np.arange(first_sample_count + 1, first_sample_count + n_frames + 1, dtype=np.float32)
    return (np.float32(seed_step) * k).astype(np.float32)


# ----------------------------------------------------------------------------------------------
# PathTracer driver (host/path_tracer.h), as the reference's GLWidget would use it
# ----------------------------------------------------------------------------------------------

class PathTracer:
    def __init__(self, device, width, height):
        self._h = host.pbrh_pt_create(device, width, height)
        if not self._h:
            raise PbrError(host.pbrh_last_error().decode())
        self.width, self.height = width, height

    def close(self):
        if getattr(self, "_h", None):
            host.pbrh_pt_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def initOpenCLBuffers(self, scene, tile_world=1, tile_rank=0):
        if host.pbrh_pt_init(self._h, scene._h, tile_world, tile_rank) != 0:
            raise PbrError(host.pbrh_last_error().decode())

    def generateImage(self, with_debug=False):
        img = np.empty((self.height, self.width, 4), np.float32)
        dbg = np.empty_like(img) if with_debug else None
        if host.pbrh_pt_generate_image(self._h, _as_fp(img), _as_fp(dbg) if with_debug else None) != 0:
            raise PbrError(host.pbrh_last_error().decode())
        return (img, dbg) if with_debug else img

    def generateImages(self, frames):
        img = np.empty((self.height, self.width, 4), np.float32)
        if host.pbrh_pt_generate_images(self._h, frames, _as_fp(img)) != 0:
            raise PbrError(host.pbrh_last_error().decode())
        return img

    def generateImagesAdaptive(self, min_frames, round_frames, max_frames, threshold):
        """PathTracer::generateImagesAdaptive: up to max_frames frames, tiles stop once converged (Device.render_adaptive).
        Starts a new accumulation and leaves the sample count at 0: the image has a sample count per tile."""
        img = np.empty((self.height, self.width, 4), np.float32)
        if host.pbrh_pt_generate_images_adaptive(self._h, min_frames, round_frames, max_frames, threshold, _as_fp(img)) != 0:
            raise PbrError(host.pbrh_last_error().decode())
        return img

    def updateVertices(self, vertices):
        """PathTracer::updateVertices: Device.update_vertices on the tracer's context; starts a new accumulation."""
        vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 4)
        if host.pbrh_pt_update_vertices(self._h, _as_fp(vertices), vertices.shape[0]) != 0:
            raise PbrError(host.pbrh_last_error().decode())

    def updateGeometry(self, vertices, normals=None):
        """PathTracer::updateGeometry: Device.update_geometry on the tracer's context; starts a new accumulation."""
        vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 4)
        normals = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 4)
        if host.pbrh_pt_update_geometry(self._h, _as_fp(vertices), vertices.shape[0], None if normals is None else _as_fp(normals),
                                        0 if normals is None else normals.shape[0]) != 0:
            raise PbrError(host.pbrh_last_error().decode())

    def setParts(self, vertex_part, normal_part=None, num_parts=None):
        """PathTracer::setParts: Device.set_parts on the tracer's context."""
        vertex_part = np.ascontiguousarray(vertex_part, np.uint32).reshape(-1)
        if normal_part is not None:
            normal_part = np.ascontiguousarray(normal_part, np.uint32).reshape(-1)
        if num_parts is None:
            num_parts = int(max(vertex_part.max(initial=0), 0 if normal_part is None else normal_part.max(initial=0))) + 1
        if host.pbrh_pt_set_parts(self._h, vertex_part.ctypes.data_as(_up), vertex_part.shape[0],
                                  None if normal_part is None else normal_part.ctypes.data_as(_up),
                                  0 if normal_part is None else normal_part.shape[0], num_parts) != 0:
            raise PbrError(host.pbrh_last_error().decode())

    def updateTransforms(self, matrices):
        """PathTracer::updateTransforms: Device.update_transforms on the tracer's context; starts a new accumulation."""
        matrices = np.ascontiguousarray(matrices, np.float32).reshape(-1, 12)
        if host.pbrh_pt_update_transforms(self._h, _as_fp(matrices), matrices.shape[0]) != 0:
            raise PbrError(host.pbrh_last_error().decode())

    def setSkin(self, vertex_bones, vertex_weights, normal_bones=None, normal_weights=None, num_bones=None):
        """PathTracer::setSkin: Device.set_skin on the tracer's context."""
        vertex_bones, vertex_weights = _skin_arrays(vertex_bones, vertex_weights)
        normal_bones, normal_weights = _skin_arrays(normal_bones, normal_weights)
        if num_bones is None:
            num_bones = int(max(vertex_bones.max(initial=0), 0 if normal_bones is None else normal_bones.max(initial=0))) + 1
        if host.pbrh_pt_set_skin(self._h, vertex_bones.ctypes.data_as(_up), _as_fp(vertex_weights), vertex_bones.shape[0],
                                 None if normal_bones is None else normal_bones.ctypes.data_as(_up), None if normal_weights is None else _as_fp(normal_weights),
                                 0 if normal_bones is None else normal_bones.shape[0], num_bones) != 0:
            raise PbrError(host.pbrh_last_error().decode())

    def updateSkin(self, matrices):
        """PathTracer::updateSkin: Device.update_skin on the tracer's context; starts a new accumulation."""
        matrices = np.ascontiguousarray(matrices, np.float32).reshape(-1, 12)
        if host.pbrh_pt_update_skin(self._h, _as_fp(matrices), matrices.shape[0]) != 0:
            raise PbrError(host.pbrh_last_error().decode())

    def setMorph(self, vertex_targets, normal_targets=None):
        """PathTracer::setMorph: Device.set_morph on the tracer's context."""
        v = _morph_lists(vertex_targets, "vertex")
        n = (None, None, None) if normal_targets is None else _morph_lists(normal_targets, "normal")
        if host.pbrh_pt_set_morph(self._h, v[0].ctypes.data_as(_up), v[1].ctypes.data_as(_up), _as_fp(v[2]), None if n[0] is None else n[0].ctypes.data_as(_up),
                                  None if n[1] is None else n[1].ctypes.data_as(_up), None if n[2] is None else _as_fp(n[2]), len(vertex_targets)) != 0:
            raise PbrError(host.pbrh_last_error().decode())

    def updateMorph(self, weights):
        """PathTracer::updateMorph: Device.update_morph on the tracer's context; starts a new accumulation."""
        weights = np.ascontiguousarray(weights, np.float32).reshape(-1)
        if host.pbrh_pt_update_morph(self._h, _as_fp(weights), weights.shape[0]) != 0:
            raise PbrError(host.pbrh_last_error().decode())

    def updatePose(self, weights, matrices):
        """PathTracer::updatePose: Device.update_pose on the tracer's context; starts a new accumulation."""
        weights = np.ascontiguousarray(weights, np.float32).reshape(-1)
        matrices = np.ascontiguousarray(matrices, np.float32).reshape(-1, 12)
        if host.pbrh_pt_update_pose(self._h, _as_fp(weights), weights.shape[0], _as_fp(matrices), matrices.shape[0]) != 0:
            raise PbrError(host.pbrh_last_error().decode())

    def updateSkinDQ(self, dual_quats):
        """PathTracer::updateSkinDQ: Device.update_skin_dq on the tracer's context; starts a new accumulation."""
        dual_quats = np.ascontiguousarray(dual_quats, np.float32).reshape(-1, 8)
        if host.pbrh_pt_update_skin_dq(self._h, _as_fp(dual_quats), dual_quats.shape[0]) != 0:
            raise PbrError(host.pbrh_last_error().decode())

    def updatePoseDQ(self, weights, dual_quats):
        """PathTracer::updatePoseDQ: Device.update_pose_dq on the tracer's context; starts a new accumulation."""
        weights = np.ascontiguousarray(weights, np.float32).reshape(-1)
        dual_quats = np.ascontiguousarray(dual_quats, np.float32).reshape(-1, 8)
        if host.pbrh_pt_update_pose_dq(self._h, _as_fp(weights), weights.shape[0], _as_fp(dual_quats), dual_quats.shape[0]) != 0:
            raise PbrError(host.pbrh_last_error().decode())

    def refitOrderedWalk(self, on):
        """PathTracer::refitOrderedWalk: Device.refit_ordered_walk on the tracer's context."""
        if host.pbrh_pt_refit_ordered_walk(self._h, 1 if on else 0) != 0:
            raise PbrError(host.pbrh_last_error().decode())

    def setFocus(self, x, y):
        host.pbrh_pt_set_focus(self._h, x, y)

    def resetSampleCount(self):
        host.pbrh_pt_reset_sample_count(self._h)

    def sampleCount(self):
        return int(host.pbrh_pt_sample_count(self._h))
