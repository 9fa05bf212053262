"""The surface of pbr_update_vertices / pbr_read_bvh without a GPU: declared in the headers, exported by the three libraries,
bound with argument types by the harness — and one ABI version in header, library and harness."""
import ctypes
import os
import re
from importlib import import_module

from conftest import ROOT


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_headers_declare_the_entry_points():
    hip = _header("pbr_hip.h")
    assert "int pbr_update_vertices( pbr_ctx* ctx, const pbr_float4* vertices, uint32_t num_vertices );" in hip
    assert "int pbr_read_bvh( pbr_ctx* ctx, pbr_bvh_node* nodes_out, uint32_t capacity, uint32_t* num_nodes );" in hip
    assert "int pbr_multi_update_vertices( pbr_multi* m, const pbr_float4* vertices, uint32_t num_vertices );" in _header("pbr_multi.h")
    assert "int pbr_diag_refit_info( pbr_ctx* ctx, uint64_t out[8], double* upload_ms, char* why, size_t capacity );" in _header("pbr_hip_diag.h")


def test_libraries_export_and_harness_binds_them(pbr):
    for name in ("pbr_update_vertices", "pbr_read_bvh", "pbr_diag_refit_info"):
        assert hasattr(pbr.hip, name), "libpbrhip.so does not export %s" % name
    assert hasattr(pbr.host, "pbrh_pt_update_vertices"), "libpbrhost.so does not export pbrh_pt_update_vertices"
    multi = import_module(pbr.__name__ + ".multi")
    assert hasattr(multi.lib(), "pbr_multi_update_vertices"), "libpbrmulti.so does not export pbr_multi_update_vertices"
    vp, fp, up = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    assert pbr.hip.pbr_update_vertices.argtypes == [vp, vp, ctypes.c_uint32]
    assert pbr.hip.pbr_read_bvh.argtypes == [vp, vp, ctypes.c_uint32, up]
    assert pbr.hip.pbr_diag_refit_info.argtypes == [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.c_size_t]
    assert pbr.host.pbrh_pt_update_vertices.argtypes == [vp, fp, ctypes.c_uint32]
    assert multi.lib().pbr_multi_update_vertices.argtypes == [vp, vp, ctypes.c_uint32]
    for method in ("update_vertices", "read_bvh", "refit_info"):
        assert callable(getattr(pbr.Device, method))
    assert callable(getattr(pbr.PathTracer, "updateVertices")) and callable(getattr(multi.MultiDevice, "update_vertices"))


def test_one_abi_version_everywhere(pbr):
    declared = int(re.search(r"#define PBR_ABI_VERSION (\d+)", _header("pbr_hip.h")).group(1))
    assert declared == pbr.hip.pbr_abi_version() == pbr.ABI_VERSION
    assert declared >= 9          # pbr_update_vertices and pbr_read_bvh came with version 9


def test_null_context_is_refused_without_a_device(pbr):
    vertices = (ctypes.c_float * 4)()
    count = ctypes.c_uint32()
    assert pbr.hip.pbr_update_vertices(None, ctypes.addressof(vertices), 1) < 0
    assert pbr.hip.pbr_update_vertices(None, None, 0) < 0
    assert pbr.hip.pbr_read_bvh(None, None, 0, ctypes.byref(count)) < 0
    multi = import_module(pbr.__name__ + ".multi")
    assert multi.lib().pbr_multi_update_vertices(None, ctypes.addressof(vertices), 1) < 0
