"""The surface of pbr_render_adaptive without a GPU: declared in the headers, exported by the library, bound with argument
types by the harness and the host driver — and one ABI version in header, library and harness."""
import ctypes
import os
import re

from conftest import ROOT


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_headers_declare_the_entry_points():
    hip = _header("pbr_hip.h")
    assert re.search(r"int pbr_render_adaptive\( pbr_ctx\* ctx, uint32_t first_sample_count, const float\* seeds, float pxDim, const pbr_camera\* cam, const pbr_adaptive_params\* params \);", hip)
    assert re.search(r"int pbr_read_tile_stats\( pbr_ctx\* ctx, uint32_t\* frames, float\* error, uint32_t capacity, uint32_t\* count \);", hip)
    struct = re.search(r"typedef struct pbr_adaptive_params \{(.*?)\} pbr_adaptive_params;", hip, re.S).group(1)
    assert re.findall(r"(uint32_t|float)\s+(\w+);", struct) == [("uint32_t", "min_frames"), ("uint32_t", "round_frames"), ("uint32_t", "max_frames"), ("float", "threshold")]
    assert re.search(r"int pbr_diag_last_adaptive\( pbr_ctx\* ctx, uint32_t\* rounds, uint64_t\* units_traced, double\* fold_ms \);", _header("pbr_hip_diag.h"))


def test_library_exports_and_harness_binds_them(pbr):
    for name in ("pbr_render_adaptive", "pbr_read_tile_stats", "pbr_diag_last_adaptive"):
        assert hasattr(pbr.hip, name), "libpbrhip.so does not export %s" % name
    assert hasattr(pbr.host, "pbrh_pt_generate_images_adaptive"), "libpbrhost.so does not export pbrh_pt_generate_images_adaptive"
    vp, fp, up = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    assert pbr.hip.pbr_render_adaptive.argtypes == [vp, ctypes.c_uint32, fp, ctypes.c_float, ctypes.POINTER(pbr.Camera), ctypes.POINTER(pbr.AdaptiveParams)]
    assert pbr.hip.pbr_read_tile_stats.argtypes == [vp, up, fp, ctypes.c_uint32, up]
    assert pbr.hip.pbr_diag_last_adaptive.argtypes == [vp, up, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]
    assert pbr.host.pbrh_pt_generate_images_adaptive.argtypes == [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, fp]
    assert ctypes.sizeof(pbr.AdaptiveParams) == 16 and [f[0] for f in pbr.AdaptiveParams._fields_] == ["min_frames", "round_frames", "max_frames", "threshold"]
    for method in ("render_adaptive", "tile_stats", "last_adaptive"):
        assert callable(getattr(pbr.Device, method))
    assert callable(getattr(pbr.PathTracer, "generateImagesAdaptive"))


def test_one_abi_version_everywhere(pbr):
    declared = int(re.search(r"#define PBR_ABI_VERSION (\d+)", _header("pbr_hip.h")).group(1))
    assert declared == pbr.hip.pbr_abi_version() == pbr.ABI_VERSION
    assert declared >= 8          # pbr_render_adaptive came with version 8
