"""The surface of pbr_denoise_temporal / pbr_temporal_reset without a GPU: declared in the header, exported by the library,
bound with argument types by the harness — and one ABI version in header, library and harness."""
import ctypes
import os
import re

from conftest import ROOT

FIELDS = [("uint32_t", "max_history"), ("float", "normal_cos"), ("float", "sigma_world")]


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_header_declares_the_entry_points():
    hip = _header("pbr_hip.h")
    assert re.search(r"int pbr_temporal_reset\( pbr_ctx\* ctx \);", hip)
    assert re.search(r"int pbr_denoise_temporal\( pbr_ctx\* ctx, float pxDim, const pbr_camera\* cam,\s*"
                     r"const pbr_temporal_params\* temporal, const pbr_denoise_guided_params\* filter,\s*"
                     r"float\* rgba, float\* variance_out, float\* integrated, float\* history \);", hip)
    struct = re.search(r"typedef struct pbr_temporal_params \{(.*?)\} pbr_temporal_params;", hip, re.S).group(1)
    assert re.findall(r"(uint32_t|float)\s+(\w+);", struct) == FIELDS
    # the guided filter's call is as it was
    assert re.search(r"int pbr_denoise_guided\( pbr_ctx\* ctx, float pxDim, const pbr_camera\* cam, const pbr_denoise_guided_params\* params,\s*"
                     r"float\* rgba, float\* variance_out, float\* features \);", hip)


def test_library_exports_and_harness_binds_them(pbr):
    for name in ("pbr_temporal_reset", "pbr_denoise_temporal"):
        assert hasattr(pbr.hip, name), "libpbrhip.so does not export %s" % name
    vp, fp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)
    assert pbr.hip.pbr_temporal_reset.argtypes == [vp]
    assert pbr.hip.pbr_denoise_temporal.argtypes == [vp, ctypes.c_float, ctypes.POINTER(pbr.Camera), ctypes.POINTER(pbr.TemporalParams),
                                                     ctypes.POINTER(pbr.GuidedDenoiseParams), fp, fp, fp, fp]
    assert ctypes.sizeof(pbr.TemporalParams) == 12
    assert [f[0] for f in pbr.TemporalParams._fields_] == [name for _, name in FIELDS]
    p = pbr.TemporalParams()
    assert (p.max_history, p.normal_cos, p.sigma_world) == (32, ctypes.c_float(0.9).value, 3.0)
    for method in ("denoise_temporal", "temporal_reset"):
        assert callable(getattr(pbr.Device, method))


def test_one_abi_version_everywhere(pbr):
    declared = int(re.search(r"#define PBR_ABI_VERSION (\d+)", _header("pbr_hip.h")).group(1))
    assert declared == pbr.hip.pbr_abi_version() == pbr.ABI_VERSION
    assert declared >= 11         # pbr_denoise_temporal and pbr_temporal_reset came with version 11
