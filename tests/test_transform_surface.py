"""The surface of pbr_set_parts / pbr_update_transforms / pbr_read_geometry without a GPU: declared in the headers with the
definition stated in full, exported by every library that exports pbr_update_geometry, bound with argument types by the
harness, forwarded by PathTracer, one ABI version in header, library and harness, and refused for a null context."""
import ctypes
import os
import re

from conftest import ROOT

SYMBOLS = ("pbr_set_parts", "pbr_update_transforms", "pbr_read_geometry", "pbr_diag_transform_info")


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_headers_declare_the_entry_points_and_state_the_definition():
    hip = _header("pbr_hip.h")
    start = hip.index("int pbr_update_geometry( pbr_ctx* ctx, const pbr_float4* vertices, uint32_t num_vertices,")
    parts = hip.index("int pbr_set_parts( pbr_ctx* ctx, const uint32_t* vertex_part, uint32_t num_vertices, const uint32_t* normal_part, uint32_t num_normals,")
    assert "uint32_t num_parts );" in hip[parts:parts + 220]
    assert "int pbr_update_transforms( pbr_ctx* ctx, const float* matrices, uint32_t num_parts );" in hip
    read = hip.index("int pbr_read_geometry( pbr_ctx* ctx, pbr_float4* vertices_out, uint32_t vcap, uint32_t* num_vertices,")
    assert "pbr_float4* normals_out, uint32_t ncap, uint32_t* num_normals );" in hip[read:read + 220]
    # the calls that were there keep their signatures
    assert "int pbr_update_vertices( pbr_ctx* ctx, const pbr_float4* vertices, uint32_t num_vertices );" in hip
    assert "int pbr_read_bvh( pbr_ctx* ctx, pbr_bvh_node* nodes_out, uint32_t capacity, uint32_t* num_nodes );" in hip
    contract = re.sub(r"\s*\n \*\s+", " ", hip[start:parts])
    for phrase in ("ABI version 15", "REST POSE", "row-major 3 x 4", "m[4r+3] the translation", "it is not cumulative",
                   "c0 = cross( a1, a2 ), c1 = cross( a2, a0 ), c2 = cross( a0, a1 ), det = dot( a0, c0 )",
                   "if det < 0 every word of c0, c1, c2 is negated", "p'.x = ( ( m0*p.x + m1*p.y ) + m2*p.z ) + m3", "p'.w = p.w bit for bit",
                   "q.r = dot( c_r, n ), d = dot( q, q )", "q * ( 1.0f / sqrtf( d ) )", "no normal word is ever NaN", "correctly rounded",
                   "compare equal, as floats, to the identity", "THE CONTRACT", "pbr_update_geometry( V', N' )", "the message names pbr_set_parts",
                   "found ON THE DEVICE", "the two pointers are swapped", "ALL allocation happens in this call", "OUT OF SCOPE: pbr_multi.h",
                   "per-vertex skinning"):
        assert phrase in contract, phrase
    assert "version 15 pbr_set_parts, pbr_update_transforms" in hip
    assert "int pbr_diag_transform_info( pbr_ctx* ctx, uint64_t out[4], double* ms );" in _header("pbr_hip_diag.h")


def test_every_library_that_exports_update_geometry_exports_them(pbr):
    from importlib import import_module
    build = import_module(pbr.__name__ + ".build")
    checked = 0
    for path in (build.HIP_LIB, build.HIP_GUARD_LIB):
        if os.path.exists(path):
            lib = ctypes.CDLL(path)
            assert hasattr(lib, "pbr_update_geometry")
            for name in SYMBOLS:
                assert hasattr(lib, name), "%s does not export %s" % (path, name)
            checked += 1
    assert checked >= 1
    assert hasattr(pbr.host, "pbrh_pt_update_geometry")
    for name in ("pbrh_pt_set_parts", "pbrh_pt_update_transforms"):
        assert hasattr(pbr.host, name), "libpbrhost.so does not export %s" % name


def test_harness_binds_them_with_argument_types(pbr):
    vp, u32, up, fp = ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float)
    assert pbr.hip.pbr_set_parts.argtypes == [vp, vp, u32, vp, u32, u32]
    assert pbr.hip.pbr_update_transforms.argtypes == [vp, vp, u32]
    assert pbr.hip.pbr_read_geometry.argtypes == [vp, vp, u32, up, vp, u32, up]
    assert pbr.hip.pbr_diag_transform_info.argtypes == [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]
    assert pbr.host.pbrh_pt_set_parts.argtypes == [vp, up, u32, up, u32, u32]
    assert pbr.host.pbrh_pt_update_transforms.argtypes == [vp, fp, u32]
    for method in ("set_parts", "update_transforms", "read_geometry", "transform_info"):
        assert callable(getattr(pbr.Device, method))
    for method in ("setParts", "updateTransforms"):
        assert callable(getattr(pbr.PathTracer, method))


def test_the_loader_reaches_the_forwarders():
    import pbr_loader
    pbr = pbr_loader.load()
    assert callable(pbr.Device.update_transforms) and callable(pbr.Device.read_geometry)


def test_one_abi_version_everywhere(pbr):
    declared = int(re.search(r"#define PBR_ABI_VERSION (\d+)", _header("pbr_hip.h")).group(1))
    assert declared == pbr.hip.pbr_abi_version() == pbr.ABI_VERSION
    assert declared >= 15         # the transforms came with version 15


def test_null_context_is_refused_without_a_device(pbr):
    words = (ctypes.c_uint32 * 4)()
    matrix = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    out, ms, count = (ctypes.c_uint64 * 4)(), ctypes.c_double(), ctypes.c_uint32()
    assert pbr.hip.pbr_set_parts(None, ctypes.addressof(words), 4, None, 0, 1) == -1
    assert pbr.hip.pbr_set_parts(None, None, 0, None, 0, 0) == -1
    assert pbr.hip.pbr_update_transforms(None, ctypes.addressof(matrix), 1) == -1
    assert pbr.hip.pbr_read_geometry(None, None, 0, ctypes.byref(count), None, 0, ctypes.byref(count)) == -1
    assert pbr.hip.pbr_diag_transform_info(None, out, ctypes.byref(ms)) == -1
