// pt_denoise_host.hpp — the host side of pbr_denoise, pbr_denoise_guided and pbr_denoise_temporal (pbr_hip.hip) that needs no
// device: the arguments their kernels take by value, what the calls refuse, the a-trous pass schedule, and the camera terms
// the launches are set up with.  Host code only, no HIP: tests/denoise_host_driver.cpp builds it with a plain C++17 compiler
// and -ffp-contract=off, as the library is built — every expression below is the sequence of binary32 operations the kernels'
// definitions (include/pbr_hip.h) and the numpy restatements (tests/guided_denoise_ref.py, tests/temporal_ref.py) assume.
#pragma once

#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "pbr_hip.h"

namespace ptd {

// ---- what the kernels take by value (pt_denoise.hpp, pt_denoise_guided.hpp, pt_temporal.hpp) ----

struct DenoiseArgs {
	int width, height, step;
	float invColor;     // 1 / sigma_color_k^2 of this pass, 0 = off
	float invNormal;    // 1 / sigma_normal^2, 0 = off
	float invAlbedo;    // 1 / sigma_albedo^2, 0 = off
	float worldScale;   // sigma_world * step * pxDim: times the centre's distance = the standard deviation in world units; 0 = off
};

struct GuidedArgs {
	int width, height, step;
	float sigmaLuminance;   // in standard deviations of the pixel's mean, 0 = off
	float invNormal;        // as DenoiseArgs
	float invAlbedo;
	float worldScale;
};

struct TemporalArgs {
	int width, height;
	int hasHistory;          // 0: the first call after a reset — no pixel has a candidate
	unsigned maxHistory;
	float normalCos;
	int worldTerm;           // sigma_world != 0: the distance term is on
	float worldScale;        // sigma_world * pxDim of this call
	// the previous call's camera
	float eye[3], cu[3], cv[3], cw[3];
	float halfPx;
	// this call's camera as setCamera lays it out (centreRay's terms), for the miss pixels
	float curCu[3], curCv[3], curCw[3], curCamA[3], curCvH[3];
	float curHalfPx;
};

// ---- what the calls refuse: PBR_EINVAL with the message in *why, or PBR_OK.  `who` is the entry point's name ----

inline int refuse( std::string* why, const char* who, const std::string& what ) {
	*why = std::string( who ) + ": " + what;
	return PBR_EINVAL;
}

inline bool finiteNotNegative( float sigma ) {
	return sigma >= 0.0f && std::isfinite( sigma );
}

inline float firstSigma( const pbr_denoise_params& p ) { return p.sigma_color; }
inline float firstSigma( const pbr_denoise_guided_params& p ) { return p.sigma_luminance; }

// a filter's {passes, four standard deviations}: pbr_denoise_params or pbr_denoise_guided_params
template <class Params>
int filterCheck( const char* who, const Params& params, std::string* why ) {
	if( params.passes < 1 || params.passes > 8 ) {
		return refuse( why, who, "1 .. 8 passes (got " + std::to_string( params.passes ) + ")" );
	}

	for( float sigma : { firstSigma( params ), params.sigma_normal, params.sigma_world, params.sigma_albedo } ) {
		if( !finiteNotNegative( sigma ) ) {
			return refuse( why, who, "the filter's standard deviations must be finite and >= 0 (0 switches a term off)" );
		}
	}

	return PBR_OK;
}

inline int temporalCheck( const char* who, const pbr_temporal_params& temporal, std::string* why ) {
	if( temporal.max_history < 1 || temporal.max_history > 1024 ) {
		return refuse( why, who, "max_history 1 .. 1024 (got " + std::to_string( temporal.max_history ) + ")" );
	}
	if( !( temporal.normal_cos >= -1.0f && temporal.normal_cos <= 1.0f ) ) {
		return refuse( why, who, "normal_cos must be in [-1, 1]" );
	}
	if( !finiteNotNegative( temporal.sigma_world ) ) {
		return refuse( why, who, "sigma_world must be finite and >= 0 (0 switches the term off)" );
	}

	return PBR_OK;
}

// pbr_denoise, pbr_denoise_guided
template <class Params>
int denoiseCheck( const char* who, const pbr_camera* cam, const Params* params, const float* rgba, std::string* why ) {
	if( cam == nullptr || params == nullptr || rgba == nullptr ) {
		return refuse( why, who, "null camera, parameters or destination" );
	}

	return filterCheck( who, *params, why );
}

// pbr_denoise_temporal: the history's parameters first, then the filter's
inline int denoiseTemporalCheck( const char* who, const pbr_camera* cam, const pbr_temporal_params* temporal, const pbr_denoise_guided_params* filter,
                                 const float* rgba, std::string* why ) {
	if( cam == nullptr || temporal == nullptr || filter == nullptr || rgba == nullptr ) {
		return refuse( why, who, "null camera, parameters or destination" );
	}

	const int status = temporalCheck( who, *temporal, why );
	return ( status != PBR_OK ) ? status : filterCheck( who, *filter, why );
}

// ---- the pass schedule: pass k = 0 .. passes - 1 of a w x h image, taps 2^k pixels apart ----

inline float inverseSquare( float sigma ) {
	return ( sigma > 0.0f ) ? 1.0f / ( sigma * sigma ) : 0.0f;
}

// the colour's standard deviation halves from pass to pass (Dammertz et al. 2010, section 3.3): what the early passes
// smoothed, the late, wide ones must not blur again
inline DenoiseArgs plainPass( const pbr_denoise_params& params, uint32_t pass, int w, int h, float pxDim ) {
	const int step = 1 << pass;
	return DenoiseArgs{ w, h, step, inverseSquare( params.sigma_color / (float) ( 1u << pass ) ), inverseSquare( params.sigma_normal ),
		inverseSquare( params.sigma_albedo ), ( params.sigma_world * (float) step ) * pxDim };
}

inline GuidedArgs guidedPass( const pbr_denoise_guided_params& params, uint32_t pass, int w, int h, float pxDim ) {
	const int step = 1 << pass;
	return GuidedArgs{ w, h, step, params.sigma_luminance, inverseSquare( params.sigma_normal ), inverseSquare( params.sigma_albedo ),
		( params.sigma_world * (float) step ) * pxDim };
}

// ---- the camera of a w x h image: its vectors, and the launch-invariant sub-expressions of initRay (pt_kernel.hpp) and
// centreRay (pt_denoise.hpp) in the same IEEE single operations as the kernel would do ----

struct CameraTerms {
	float eye[3], cu[3], cv[3], cw[3];
	float camA[3];   // cu - cu * w
	float cvH[3];    // cv * h
	float halfPx, pxDim;
};

inline void copy3( float* dst, const float* src ) {
	dst[0] = src[0];
	dst[1] = src[1];
	dst[2] = src[2];
}

inline CameraTerms cameraTerms( const pbr_camera& cam, int w, int h, float pxDim ) {
	CameraTerms T;
	copy3( T.eye, &cam.eye.x );
	copy3( T.cu, &cam.u.x );
	copy3( T.cv, &cam.v.x );
	copy3( T.cw, &cam.w.x );

	for( int k = 0; k < 3; k++ ) {
		const float cuW = T.cu[k] * (float) w;
		T.camA[k] = T.cu[k] - cuW;
		T.cvH[k] = T.cv[k] * (float) h;
	}

	T.halfPx = pxDim * 0.5f;
	T.pxDim = pxDim;
	return T;
}

// temporalIntegrate's arguments: the history's camera (oldCam, oldPxDim — whatever they hold while there is no history) and
// this call's, cur = cameraTerms( cam, w, h, pxDim )
inline TemporalArgs temporalArgs( const pbr_temporal_params& temporal, int w, int h, float pxDim, bool hasHistory, const pbr_camera& oldCam,
                                  float oldPxDim, const CameraTerms& cur ) {
	TemporalArgs T;
	T.width = w;
	T.height = h;
	T.hasHistory = hasHistory ? 1 : 0;
	T.maxHistory = temporal.max_history;
	T.normalCos = temporal.normal_cos;
	T.worldTerm = ( temporal.sigma_world != 0.0f ) ? 1 : 0;
	T.worldScale = temporal.sigma_world * pxDim;
	copy3( T.eye, &oldCam.eye.x );
	copy3( T.cu, &oldCam.u.x );
	copy3( T.cv, &oldCam.v.x );
	copy3( T.cw, &oldCam.w.x );
	T.halfPx = oldPxDim * 0.5f;
	copy3( T.curCu, cur.cu );
	copy3( T.curCv, cur.cv );
	copy3( T.curCw, cur.cw );
	copy3( T.curCamA, cur.camA );
	copy3( T.curCvH, cur.cvH );
	T.curHalfPx = cur.halfPx;
	return T;
}

}  // namespace ptd
