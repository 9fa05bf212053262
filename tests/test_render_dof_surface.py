"""The surface of pbr_render_dof without a GPU: declared in the headers, exported by the library, bound with argument types
by the harness — and one ABI version in header, library and harness (a new entry point is an ABI change)."""
import ctypes
import os
import re

from conftest import ROOT


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_headers_declare_the_entry_points():
    assert re.search(r"int pbr_render_dof\( pbr_ctx\* ctx, uint32_t first_sample_count, uint32_t n_frames, const float\* seeds, float pxDim, const pbr_camera\* cam \);", _header("pbr_hip.h"))
    assert re.search(r"int pbr_diag_last_focus_chain\( pbr_ctx\* ctx, double\* ms \);", _header("pbr_hip_diag.h"))
    assert "pbr_render_dof" in _header("pbr_multi.h")


def test_library_exports_and_harness_binds_them(pbr):
    for name in ("pbr_render_dof", "pbr_diag_last_focus_chain"):
        assert hasattr(pbr.hip, name), "libpbrhip.so does not export %s" % name
    vp, fp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)
    assert pbr.hip.pbr_render_dof.argtypes == [vp, ctypes.c_uint32, ctypes.c_uint32, fp, ctypes.c_float, ctypes.POINTER(pbr.Camera)]
    assert pbr.hip.pbr_diag_last_focus_chain.argtypes == [vp, ctypes.POINTER(ctypes.c_double)]
    assert callable(getattr(pbr.Device, "render_dof")) and callable(getattr(pbr.Device, "last_focus_chain_ms"))


def test_one_abi_version_everywhere(pbr):
    declared = int(re.search(r"#define PBR_ABI_VERSION (\d+)", _header("pbr_hip.h")).group(1))
    assert declared == pbr.hip.pbr_abi_version() == pbr.ABI_VERSION
    assert declared >= 7          # pbr_render_dof came with version 7


def test_every_mode_has_its_chained_kernels_and_its_focus_chain(pbr):
    """pbr_mode_built counts the chained builds of a mode's plans and the mode's focus chain: a library without them does not
    claim the mode."""
    for traversal in (0, 1, 2, 3):
        for arith in (0, 1):
            assert pbr.hip.pbr_mode_built(traversal, arith) == 1, (traversal, arith)
