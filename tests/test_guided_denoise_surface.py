"""The surface of pbr_read_variance / pbr_denoise_guided without a GPU: declared in the header, exported by the library,
bound with argument types by the harness — and one ABI version in header, library and harness."""
import ctypes
import os
import re

from conftest import ROOT

FIELDS = [("uint32_t", "passes"), ("float", "sigma_luminance"), ("float", "sigma_normal"), ("float", "sigma_world"), ("float", "sigma_albedo")]


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_header_declares_the_entry_points():
    hip = _header("pbr_hip.h")
    assert re.search(r"int pbr_read_variance\( pbr_ctx\* ctx, float\* variance \);", hip)
    assert re.search(r"int pbr_denoise_guided\( pbr_ctx\* ctx, float pxDim, const pbr_camera\* cam, const pbr_denoise_guided_params\* params,\s*"
                     r"float\* rgba, float\* variance_out, float\* features \);", hip)
    struct = re.search(r"typedef struct pbr_denoise_guided_params \{(.*?)\} pbr_denoise_guided_params;", hip, re.S).group(1)
    assert re.findall(r"(uint32_t|float)\s+(\w+);", struct) == FIELDS
    # the plain filter's struct and call are as they were
    assert re.search(r"int pbr_denoise\( pbr_ctx\* ctx, float pxDim, const pbr_camera\* cam, const pbr_denoise_params\* params, float\* rgba, float\* features \);", hip)


def test_library_exports_and_harness_binds_them(pbr):
    for name in ("pbr_read_variance", "pbr_denoise_guided"):
        assert hasattr(pbr.hip, name), "libpbrhip.so does not export %s" % name
    vp, fp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)
    assert pbr.hip.pbr_read_variance.argtypes == [vp, fp]
    assert pbr.hip.pbr_denoise_guided.argtypes == [vp, ctypes.c_float, ctypes.POINTER(pbr.Camera), ctypes.POINTER(pbr.GuidedDenoiseParams), fp, fp, fp]
    assert ctypes.sizeof(pbr.GuidedDenoiseParams) == 20
    assert [f[0] for f in pbr.GuidedDenoiseParams._fields_] == [name for _, name in FIELDS]
    p = pbr.GuidedDenoiseParams()
    assert (p.passes, p.sigma_luminance, p.sigma_normal, p.sigma_world, p.sigma_albedo) == (5, 4.0, 0.25, 3.0, ctypes.c_float(0.1).value)
    for method in ("read_variance", "denoise_guided"):
        assert callable(getattr(pbr.Device, method))


def test_one_abi_version_everywhere(pbr):
    declared = int(re.search(r"#define PBR_ABI_VERSION (\d+)", _header("pbr_hip.h")).group(1))
    assert declared == pbr.hip.pbr_abi_version() == pbr.ABI_VERSION
    assert declared >= 10         # pbr_read_variance and pbr_denoise_guided came with version 10
