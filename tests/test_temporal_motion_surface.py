"""The surface of pbr_temporal_track_motion / pbr_read_temporal_motion without a GPU: declared in the header, exported by the
library, bound with argument types by the harness, ABI version 12 in header, library and harness, and -1 for a null context."""
import ctypes
import os
import re

from conftest import ROOT


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_header_declares_the_entry_points():
    hip = _header("pbr_hip.h")
    assert re.search(r"int pbr_temporal_track_motion\( pbr_ctx\* ctx, int on \);", hip)
    assert re.search(r"int pbr_read_temporal_motion\( pbr_ctx\* ctx, float\* motion, int32_t\* face \);", hip)
    # pbr_denoise_temporal keeps its signature
    assert re.search(r"int pbr_denoise_temporal\( pbr_ctx\* ctx, float pxDim, const pbr_camera\* cam,\s*"
                     r"const pbr_temporal_params\* temporal, const pbr_denoise_guided_params\* filter,\s*"
                     r"float\* rgba, float\* variance_out, float\* integrated, float\* history \);", hip)


def test_library_exports_and_harness_binds_them(pbr):
    for name in ("pbr_temporal_track_motion", "pbr_read_temporal_motion"):
        assert hasattr(pbr.hip, name), "libpbrhip.so does not export %s" % name
    vp, fp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)
    assert pbr.hip.pbr_temporal_track_motion.argtypes == [vp, ctypes.c_int]
    assert pbr.hip.pbr_read_temporal_motion.argtypes == [vp, fp, ctypes.POINTER(ctypes.c_int32)]
    for method in ("temporal_track_motion", "temporal_motion"):
        assert callable(getattr(pbr.Device, method))


def test_abi_version_12_everywhere(pbr):
    declared = int(re.search(r"#define PBR_ABI_VERSION (\d+)", _header("pbr_hip.h")).group(1))
    assert declared == pbr.hip.pbr_abi_version() == pbr.ABI_VERSION
    assert declared >= 12         # pbr_temporal_track_motion and pbr_read_temporal_motion came with version 12


def test_null_context_calls_return_einval(pbr):
    motion, face = (ctypes.c_float * 4)(), (ctypes.c_int32 * 1)()
    assert pbr.hip.pbr_temporal_track_motion(None, 1) == -1
    assert pbr.hip.pbr_temporal_track_motion(None, 0) == -1
    assert pbr.hip.pbr_read_temporal_motion(None, motion, face) == -1
    assert pbr.hip.pbr_read_temporal_motion(None, None, None) == -1
