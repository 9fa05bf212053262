"""The surface of pbr_refit_ordered_walk without a GPU: declared in the headers with its contract, exported by the three
libraries, bound with argument types by the harness, forwarded by the multi-GPU driver and PathTracer, ABI version 13 in
header, library and harness, and refused for a null context."""
import ctypes
import os
import re
from importlib import import_module

from conftest import ROOT


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_headers_declare_the_entry_points_and_state_the_contract():
    hip = _header("pbr_hip.h")
    assert "int pbr_refit_ordered_walk( pbr_ctx* ctx, int on );" in hip
    # next to pbr_update_vertices, which keeps its signature
    update = hip.index("int pbr_update_vertices( pbr_ctx* ctx, const pbr_float4* vertices, uint32_t num_vertices );")
    flag = hip.index("int pbr_refit_ordered_walk( pbr_ctx* ctx, int on );")
    contract = re.sub(r"\s*\n \* ", " ", hip[update:flag])
    for phrase in ("BYTE FOR BYTE", "three-call sequence", "ranking OF THE UPLOAD", "pbr_diag_read_walk", "strict compares",
                   "nothing is allocated or freed per call"):
        assert phrase in contract, phrase
    assert "int pbr_multi_refit_ordered_walk( pbr_multi* m, int on );" in _header("pbr_multi.h")
    diag = _header("pbr_hip_diag.h")
    assert "int pbr_diag_read_walk( pbr_ctx* ctx, void* out, uint64_t capacity, uint64_t* bytes, int first[8], uint32_t* hot_slots );" in diag
    assert "int pbr_diag_relink_info( pbr_ctx* ctx, uint64_t out[4], double* ms );" in diag


def test_libraries_export_and_harness_binds_them(pbr):
    for name in ("pbr_refit_ordered_walk", "pbr_diag_read_walk", "pbr_diag_relink_info"):
        assert hasattr(pbr.hip, name), "libpbrhip.so does not export %s" % name
    assert hasattr(pbr.host, "pbrh_pt_refit_ordered_walk"), "libpbrhost.so does not export pbrh_pt_refit_ordered_walk"
    multi = import_module(pbr.__name__ + ".multi")
    assert hasattr(multi.lib(), "pbr_multi_refit_ordered_walk"), "libpbrmulti.so does not export pbr_multi_refit_ordered_walk"
    vp, up = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)
    assert pbr.hip.pbr_refit_ordered_walk.argtypes == [vp, ctypes.c_int]
    assert pbr.hip.pbr_diag_read_walk.argtypes == [vp, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int), up]
    assert pbr.hip.pbr_diag_relink_info.argtypes == [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]
    assert pbr.host.pbrh_pt_refit_ordered_walk.argtypes == [vp, ctypes.c_int]
    assert multi.lib().pbr_multi_refit_ordered_walk.argtypes == [vp, ctypes.c_int]
    for method in ("refit_ordered_walk", "read_walk", "relink_info"):
        assert callable(getattr(pbr.Device, method))
    assert callable(getattr(pbr.PathTracer, "refitOrderedWalk")) and callable(getattr(multi.MultiDevice, "refit_ordered_walk"))


def test_the_loader_reaches_the_forwarders():
    import pbr_loader
    pbr = pbr_loader.load()
    assert callable(pbr.Device.refit_ordered_walk)


def test_abi_version_13_everywhere(pbr):
    declared = int(re.search(r"#define PBR_ABI_VERSION (\d+)", _header("pbr_hip.h")).group(1))
    assert declared == pbr.hip.pbr_abi_version() == pbr.ABI_VERSION
    assert declared >= 13         # pbr_refit_ordered_walk came with version 13
    assert "version 13 pbr_refit_ordered_walk" in _header("pbr_hip.h")


def test_null_context_is_refused_without_a_device(pbr):
    size, first, hot = ctypes.c_uint64(), (ctypes.c_int * 8)(), ctypes.c_uint32()
    out = (ctypes.c_uint64 * 4)()
    assert pbr.hip.pbr_refit_ordered_walk(None, 1) == -1
    assert pbr.hip.pbr_refit_ordered_walk(None, 0) == -1
    assert pbr.hip.pbr_diag_read_walk(None, None, 0, ctypes.byref(size), first, ctypes.byref(hot)) == -1
    assert pbr.hip.pbr_diag_relink_info(None, out, None) == -1
    multi = import_module(pbr.__name__ + ".multi")
    assert multi.lib().pbr_multi_refit_ordered_walk(None, 1) == -1
