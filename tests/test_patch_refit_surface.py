"""The surface of pbr_update_geometry without a GPU: declared in the headers with the face box stated in full, exported by the
libraries, bound with argument types by the harness, forwarded by PathTracer, ABI version 14 in header, library and harness,
and refused for a null context."""
import ctypes
import os
import re

from conftest import ROOT


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_headers_declare_the_entry_points_and_state_the_definition():
    hip = _header("pbr_hip.h")
    flag = hip.index("int pbr_refit_ordered_walk( pbr_ctx* ctx, int on );")
    call = hip.index("int pbr_update_geometry( pbr_ctx* ctx, const pbr_float4* vertices, uint32_t num_vertices,")
    assert "const pbr_float4* normals, uint32_t num_normals );" in hip[call:call + 200]
    # pbr_update_vertices keeps its signature
    assert "int pbr_update_vertices( pbr_ctx* ctx, const pbr_float4* vertices, uint32_t num_vertices );" in hip
    contract = re.sub(r"\s*\n \*\s+", " ", hip[flag:call])
    for phrase in ("ABI version 14", "six quads", "lo = hi = p1", "( v < lo ) ? v : lo", "fabsf( t.k ) > 0.000001f", "p_k + thickness * ng",
                   "( 0, .5 ) ( .5, 0 ) ( .5, .5 ) ( .25, .75 ) ( .75, .25 ) ( .25, 0 ) ( .75, 0 ) ( 0, .25 ) ( 0, .75 )",
                   "( a.x*b.x + a.y*b.y ) + a.z*b.z", "a * ( 1.0f / sqrtf( dot( a, a ) ) )", "w = ( 1.0f - u ) - v", "correctly rounded",
                   "A NaN point never enters the fold", "ONE running fold", "With alpha = 0 every box is, bit for bit, pbr_update_vertices's",
                   "THE STATE RULE", "compared as floats", "Nothing is allocated per call"):
        assert phrase in contract, phrase
    diag = _header("pbr_hip_diag.h")
    assert "int pbr_diag_patch_refit_info( pbr_ctx* ctx, uint64_t out[4], float* alpha );" in diag
    assert "int pbr_diag_read_patches( pbr_ctx* ctx, pbr_float4* out, uint32_t capacity, uint32_t* count );" in diag


def test_libraries_export_and_harness_binds_them(pbr):
    for name in ("pbr_update_geometry", "pbr_diag_patch_refit_info", "pbr_diag_read_patches"):
        assert hasattr(pbr.hip, name), "libpbrhip.so does not export %s" % name
    assert hasattr(pbr.host, "pbrh_pt_update_geometry"), "libpbrhost.so does not export pbrh_pt_update_geometry"
    vp, up, fp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float)
    assert pbr.hip.pbr_update_geometry.argtypes == [vp, vp, ctypes.c_uint32, vp, ctypes.c_uint32]
    assert pbr.hip.pbr_diag_patch_refit_info.argtypes == [vp, ctypes.POINTER(ctypes.c_uint64), fp]
    assert pbr.hip.pbr_diag_read_patches.argtypes == [vp, vp, ctypes.c_uint32, up]
    assert pbr.host.pbrh_pt_update_geometry.argtypes == [vp, fp, ctypes.c_uint32, fp, ctypes.c_uint32]
    for method in ("update_geometry", "read_patches", "patch_refit_info"):
        assert callable(getattr(pbr.Device, method))
    assert callable(getattr(pbr.PathTracer, "updateGeometry"))


def test_the_loader_reaches_the_forwarders():
    import pbr_loader
    pbr = pbr_loader.load()
    assert callable(pbr.Device.update_geometry)


def test_abi_version_14_everywhere(pbr):
    declared = int(re.search(r"#define PBR_ABI_VERSION (\d+)", _header("pbr_hip.h")).group(1))
    assert declared == pbr.hip.pbr_abi_version() == pbr.ABI_VERSION
    assert declared >= 14         # pbr_update_geometry came with version 14
    assert "version 14 pbr_update_geometry" in _header("pbr_hip.h")


def test_null_context_is_refused_without_a_device(pbr):
    vertices = (ctypes.c_float * 4)()
    out, alpha, count = (ctypes.c_uint64 * 4)(), ctypes.c_float(), ctypes.c_uint32()
    assert pbr.hip.pbr_update_geometry(None, ctypes.addressof(vertices), 1, ctypes.addressof(vertices), 1) == -1
    assert pbr.hip.pbr_update_geometry(None, None, 0, None, 0) == -1
    assert pbr.hip.pbr_diag_patch_refit_info(None, out, ctypes.byref(alpha)) == -1
    assert pbr.hip.pbr_diag_read_patches(None, None, 0, ctypes.byref(count)) == -1
