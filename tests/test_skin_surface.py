"""The surface of pbr_set_skin / pbr_update_skin without a GPU: declared in the headers with the definition stated in full,
exported by every library that exports pbr_update_geometry, bound with argument types by the harness, forwarded by PathTracer,
one ABI version in header, library and harness, and refused for a null context."""
import ctypes
import os
import re

from conftest import ROOT

SYMBOLS = ("pbr_set_skin", "pbr_update_skin", "pbr_diag_skin_info")


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_headers_declare_the_entry_points_and_state_the_definition():
    hip = _header("pbr_hip.h")
    start = hip.index("int pbr_update_transforms( pbr_ctx* ctx, const float* matrices, uint32_t num_parts );")
    skin = hip.index("int pbr_set_skin( pbr_ctx* ctx, const uint32_t* vertex_bones, const float* vertex_weights, uint32_t num_vertices,")
    assert start < skin                                              # the new block stands behind pbr_update_transforms' declaration
    assert "const uint32_t* normal_bones, const float* normal_weights, uint32_t num_normals, uint32_t num_bones );" in hip[skin:skin + 260]
    assert "int pbr_update_skin( pbr_ctx* ctx, const float* matrices, uint32_t num_bones );" in hip
    assert "#define PBR_SKIN_INFLUENCES 4" in hip
    # the calls that were there keep their signatures
    assert "int pbr_update_transforms( pbr_ctx* ctx, const float* matrices, uint32_t num_parts );" in hip
    assert "uint32_t num_parts );" in hip[hip.index("int pbr_set_parts("):][:220]
    contract = re.sub(r"\s*\n \*\s+", " ", hip[start:skin])
    for phrase in ("ABI version 16", "REST POSE", "vertex_bones[4*i + j] and vertex_weights[4*i + j] are slot j of vertex i", "pbr_update_transforms' layout",
                   "it never accumulates", "whose weight compares unequal to 0, in slot order", "contributes nothing, not even a +0",
                   "an unused slot may name any valid bone", "B[k] = w_s * m_s[k]", "B[k] = B[k] + w_s * m_s[k]", "a product and then an addition",
                   "p'.x = ( ( B0*p.x + B1*p.y ) + B2*p.z ) + B3", "p'.w = p.w bit for bit", "compare equal, as floats, to the identity",
                   "c0 = cross( a1, a2 ), c1 = cross( a2, a0 ), c2 = cross( a0, a1 ), det = dot( a0, c0 )", "negated if det < 0",
                   "transformNormal( c, isIdentity( B ), n )", "a d that is 0, infinite or NaN copies the rest normal", "a singular blend is legal",
                   "no normal word is ever NaN", "THE WEIGHTS ARE USED AS GIVEN", "not normalised and their sum is not checked",
                   "ONE-HOT SKIN EQUALS THE RIGID CALL", "1.0f * x is x, -0 stays -0", "UNMOVED ELEMENTS STAY UNMOVED", "NOT PROMISED",
                   "THE CONTRACT", "pbr_update_geometry( V', N' )", "the message names pbr_set_skin", "found ON THE DEVICE", "only then the pointers are swapped",
                   "the normals are written after that check", "ALL allocation happens in this call", "pbr_update_skin allocates nothing",
                   "one 32-byte influence record per element", "A skin and parts are independent", "zero-weight slots included",
                   "NOT checked for a zero determinant", "pbr_diag_transform_info's last_update is 0",
                   "OUT OF SCOPE: more than four influences, dual-quaternion skinning, morph targets, pbr_multi.h, topology changes",
                   "the refit's boxes remain what pbr_read_bvh shows"):
        assert phrase in contract, phrase
    # the rigid call's out-of-scope sentence is amended, not deleted
    rigid = re.sub(r"\s*\n \*\s+", " ", hip[hip.index("int pbr_update_geometry( pbr_ctx* ctx, const pbr_float4* vertices,"):hip.index("int pbr_set_parts(")])
    assert "per-vertex skinning and blend weights (not in these two calls: pbr_set_skin and pbr_update_skin" in rigid
    assert "version 15 pbr_set_parts, pbr_update_transforms" in hip and "version 16 pbr_set_skin and pbr_update_skin" in hip
    diag = _header("pbr_hip_diag.h")
    assert "int pbr_diag_skin_info( pbr_ctx* ctx, uint64_t out[4], double* ms );" in diag
    assert "64 V + 48 N + 48 bones + 4" in diag                      # the byte formula a test computes


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
    for name in ("pbrh_pt_set_skin", "pbrh_pt_update_skin"):
        assert hasattr(pbr.host, name), "libpbrhost.so does not export %s" % name


def test_harness_binds_them_with_argument_types(pbr):
    vp, u32, up, fp = ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float)
    assert pbr.hip.pbr_set_skin.argtypes == [vp, vp, vp, u32, vp, vp, u32, u32]
    assert pbr.hip.pbr_update_skin.argtypes == [vp, vp, u32]
    assert pbr.hip.pbr_diag_skin_info.argtypes == [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]
    assert pbr.host.pbrh_pt_set_skin.argtypes == [vp, up, fp, u32, up, fp, u32, u32]
    assert pbr.host.pbrh_pt_update_skin.argtypes == [vp, fp, u32]
    for method in ("set_skin", "update_skin", "skin_info"):
        assert callable(getattr(pbr.Device, method))
    for method in ("setSkin", "updateSkin"):
        assert callable(getattr(pbr.PathTracer, method))


def test_the_loader_reaches_the_forwarders():
    import pbr_loader
    pbr = pbr_loader.load()
    assert callable(pbr.Device.update_skin) and callable(pbr.Device.set_skin) and callable(pbr.Device.skin_info)


def test_one_abi_version_everywhere(pbr):
    declared = int(re.search(r"#define PBR_ABI_VERSION (\d+)", _header("pbr_hip.h")).group(1))
    assert declared == pbr.hip.pbr_abi_version() == pbr.ABI_VERSION
    assert declared >= 16         # the skin came with version 16


def test_null_context_is_refused_without_a_device(pbr):
    bones = (ctypes.c_uint32 * 4)()
    weights = (ctypes.c_float * 4)(1, 0, 0, 0)
    matrix = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    out, ms = (ctypes.c_uint64 * 4)(), ctypes.c_double()
    assert pbr.hip.pbr_set_skin(None, ctypes.addressof(bones), ctypes.addressof(weights), 1, None, None, 0, 1) == -1
    assert pbr.hip.pbr_set_skin(None, None, None, 0, None, None, 0, 0) == -1
    assert pbr.hip.pbr_update_skin(None, ctypes.addressof(matrix), 1) == -1
    assert pbr.hip.pbr_diag_skin_info(None, out, ctypes.byref(ms)) == -1
