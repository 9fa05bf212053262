// The stage diagnostics (pt_diag.hpp) in the native arithmetic: pbr_diag_math / pbr_diag_brdf / pbr_diag_new_ray /
// pbr_diag_solve_cubic / pbr_diag_phong_face / pbr_diag_camera_ray / pbr_diag_intersect / pbr_diag_surface_step run these when the context's configuration has arith = PBR_ARITH_NATIVE (pbr_hip.hip), so the mode's math layer, BRDF
// evaluation and new-ray sampling can be held to something stage by stage, not only through images.
//   hipcc -c -DPT_FLAVOUR=2 <native flags> pt_diag_native.hip      (build.py)
#if !defined( PT_FLAVOUR ) || PT_FLAVOUR != 2
#error "pt_diag_native.hip is compiled in the native-arithmetic flavour only: -DPT_FLAVOUR=2, see build.py"
#endif

#include "pt_diag.hpp"

// stage 0: diagMath; 1: diagBrdf<brdf>; 2: diagNewRay<brdf>; 3: diagSolveCubic; 4: diagPhongFace; 5: diagCameraRay; 6: diagIntersect;
// 7: diagSurfaceStep<brdf>.  Null for an unknown stage.
extern "C" const void* pt_diag_native_pick( int stage, uint32_t brdf ) {
	switch( stage ) {
		case 0: return (const void*) ptk::diagMath;
		case 1: return ( brdf == 0 ) ? (const void*) ptk::diagBrdf<0> : (const void*) ptk::diagBrdf<1>;
		case 2: return ( brdf == 0 ) ? (const void*) ptk::diagNewRay<0> : (const void*) ptk::diagNewRay<1>;
		case 3: return (const void*) ptk::diagSolveCubic;
		case 4: return (const void*) ptk::diagPhongFace;
		case 5: return (const void*) ptk::diagCameraRay;
		case 6: return (const void*) ptk::diagIntersect;
		case 7: return ( brdf == 0 ) ? (const void*) ptk::diagSurfaceStep<0> : (const void*) ptk::diagSurfaceStep<1>;
		default: return nullptr;
	}
}
