// pt_display_host.hpp — pbr_display (include/pbr_hip.h): exposure, tone curve and transfer function between the accumulated HDR
// image and an 8-bit one.  One source for both sides: the kernels of pt_display.hpp call the three per-pixel functions below
// on the device (the bin of a pixel, the map of a channel, the encode), pbr_hip.hip calls the parameter check, the target and
// the adaptation on the host, and tests/display_driver.cpp (a plain C++17 compiler, -ffp-contract=off like the library) builds
// all of it without a device.  tests/display_ref.py restates it in numpy.
//
// Operation by operation in binary32 unless it says double, none fused (the header has it in full):
//   luminance   c' = fminf( fmaxf( c, 0 ), FLT_MAX ) per channel (NaN -> 0, inf -> FLT_MAX); Y = ( 0.2126f*r' + 0.7152f*g' ) + 0.0722f*b'
//   bin         Y == 0: dark; else clamp( (int) ( bits( Y ) >> 20 ) - 888, 0, 255 ) — eight bins per octave over [2^-16, 2^16)
//   target      double, from the 256 counts: the mean of the bin centres ( b + 0.5 ) / 8 - 16 over what the two trims keep,
//               clamped to [min_log2, max_log2]
//   adaptation  log2_used = prev + (double) adapt * ( target - prev ), or the target; exposure = (float) ( (double) key * exp2( -log2_used ) )
//   map         x = fminf( fmaxf( c * exposure, 0 ), 65504 ); the curve; y = fminf( fmaxf( y, 0 ), 1 )
//   encode      linear: (int) floorf( y * 255.0f + 0.5f ); sRGB: the number of k in 1 .. 255 with y >= kSrgbThreshold[k]
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "pt_patch_refit_host.hpp"

namespace ptv {

const int kBins = 256;
const int kDarkSlot = 256;       // where the kernels count the pixels with Y == 0, behind the bins
const int kCountSlots = 257;

// T[k], k = 1 .. 255: the smallest binary32 not below the inverse sRGB OETF of ( k - 0.5 ) / 255 evaluated in double —
// ( ( c + 0.055 ) / 1.055 )^2.4 above 0.04045, c / 12.92 below.  y >= T[k] exactly when the code of y is at least k, so no pow
// runs per pixel.  Strictly increasing; no x_k is closer than 2.8e-11 relative to a binary32, so every libm gives this table
// (tests/display_ref.py recomputes it).  Word 0 is not a threshold: the search below never reads it.
static const float kSrgbThreshold[256] = {
	0.0f, 0.000151763496f, 0.000455290487f, 0.000758817478f, 0.00106234453f, 0.00136587152f, 0.00166939851f, 0.00197292562f,
	0.00227645249f, 0.00257997937f, 0.00288350647f, 0.00318830111f, 0.00350925955f, 0.00384831498f, 0.00420574844f, 0.00458183279f,
	0.00497683743f, 0.00539102452f, 0.0058246511f, 0.00627796957f, 0.00675122766f, 0.00724466844f, 0.00775853079f, 0.00829304848f,
	0.00884845387f, 0.00942497142f, 0.0100228265f, 0.010642237f, 0.0112834219f, 0.0119465925f, 0.0126319602f, 0.0133397318f,
	0.0140701123f, 0.0148233036f, 0.0155995032f, 0.0163989104f, 0.0172217172f, 0.0180681162f, 0.0189382955f, 0.0198324434f,
	0.0207507461f, 0.0216933843f, 0.0226605386f, 0.0236523915f, 0.0246691164f, 0.0257108882f, 0.026777884f, 0.0278702714f,
	0.0289882217f, 0.0301319025f, 0.0313014835f, 0.0324971229f, 0.0337189883f, 0.0349672437f, 0.0362420455f, 0.0375435539f,
	0.038871929f, 0.04022732f, 0.0416098908f, 0.0430197865f, 0.0444571637f, 0.045922175f, 0.0474149659f, 0.048935689f,
	0.0504844859f, 0.0520615093f, 0.0536669008f, 0.055300802f, 0.0569633618f, 0.0586547181f, 0.0603750125f, 0.0621243864f,
	0.0639029741f, 0.0657109171f, 0.067548357f, 0.0694154128f, 0.0713122413f, 0.0732389614f, 0.0751957074f, 0.0771826208f,
	0.0791998208f, 0.0812474489f, 0.0833256245f, 0.085434489f, 0.0875741616f, 0.089744769f, 0.0919464454f, 0.0941793025f,
	0.0964434817f, 0.098739095f, 0.101066276f, 0.103425138f, 0.105815805f, 0.108238406f, 0.110693052f, 0.11317987f,
	0.115698971f, 0.118250489f, 0.120834522f, 0.123451203f, 0.126100644f, 0.128782958f, 0.131498262f, 0.134246677f,
	0.137028307f, 0.139843285f, 0.142691687f, 0.145573661f, 0.148489311f, 0.151438743f, 0.15442206f, 0.157439396f,
	0.160490841f, 0.163576499f, 0.166696504f, 0.169850945f, 0.173039928f, 0.176263571f, 0.179521978f, 0.182815254f,
	0.186143503f, 0.189506844f, 0.192905352f, 0.19633916f, 0.199808359f, 0.203313053f, 0.206853345f, 0.210429341f,
	0.214041144f, 0.217688859f, 0.221372575f, 0.225092396f, 0.228848428f, 0.232640773f, 0.236469522f, 0.240334779f,
	0.244236648f, 0.248175219f, 0.252150595f, 0.256162852f, 0.260212123f, 0.264298499f, 0.268422037f, 0.272582889f,
	0.276781112f, 0.281016827f, 0.285290092f, 0.289601028f, 0.293949753f, 0.298336297f, 0.30276081f, 0.30722338f,
	0.311724067f, 0.31626296f, 0.32084021f, 0.325455844f, 0.330110013f, 0.334802747f, 0.339534193f, 0.344304383f,
	0.349113464f, 0.353961498f, 0.358848572f, 0.363774806f, 0.368740231f, 0.373744994f, 0.378789157f, 0.383872777f,
	0.388996005f, 0.3941589f, 0.399361551f, 0.404604018f, 0.40988642f, 0.415208846f, 0.420571357f, 0.425974071f,
	0.431417048f, 0.436900377f, 0.442424119f, 0.447988421f, 0.453593343f, 0.459238917f, 0.464925319f, 0.47065255f,
	0.47642073f, 0.482229948f, 0.488080263f, 0.493971765f, 0.499904573f, 0.505878747f, 0.511894345f, 0.517951429f,
	0.524050176f, 0.530190587f, 0.536372721f, 0.542596757f, 0.548862696f, 0.555170655f, 0.561520696f, 0.567912936f,
	0.574347377f, 0.580824137f, 0.587343335f, 0.593905032f, 0.600509286f, 0.607156157f, 0.613845766f, 0.62057817f,
	0.62735343f, 0.634171665f, 0.641032934f, 0.647937298f, 0.654884875f, 0.661875665f, 0.668909848f, 0.675987422f,
	0.683108449f, 0.690273106f, 0.697481394f, 0.704733372f, 0.712029159f, 0.719368875f, 0.72675246f, 0.734180093f,
	0.741651833f, 0.74916774f, 0.756727874f, 0.764332294f, 0.77198118f, 0.77967447f, 0.787412345f, 0.795194805f,
	0.803021908f, 0.810893834f, 0.818810582f, 0.826772213f, 0.834778845f, 0.842830539f, 0.850927293f, 0.859069288f,
	0.867256522f, 0.875489116f, 0.883767128f, 0.892090559f, 0.900459588f, 0.908874214f, 0.917334557f, 0.925840676f,
	0.934392571f, 0.942990422f, 0.951634228f, 0.960324049f, 0.969060004f, 0.977842152f, 0.986670554f, 0.995545268f,
};

PATCH_FN uint32_t floatBits( float v ) {
	uint32_t bits;
	__builtin_memcpy( &bits, &v, sizeof( bits ) );
	return bits;
}

// fminf( fmaxf( v, 0 ), top ), written as two selects: a NaN fails both compares and becomes 0 — a signalling one too, which a
// libm's fmaxf may hand through — and -0 becomes +0, where fmaxf( -0, 0 ) may be either.  Same values otherwise.
PATCH_FN float clampTo( float v, float top ) {
	return ( v > 0.0f ) ? ( ( v < top ) ? v : top ) : 0.0f;
}

// NaN -> 0, +inf -> FLT_MAX, anything negative -> 0
PATCH_FN float countedChannel( float c ) {
	return clampTo( c, 3.40282346638528859812e+38f );
}

PATCH_FN float luminance( float r, float g, float b ) {
	return ( 0.2126f * countedChannel( r ) + 0.7152f * countedChannel( g ) ) + 0.0722f * countedChannel( b );
}

// The slot a pixel counts in: its bin, or kDarkSlot for Y == 0.  Integer arithmetic on Y's bit pattern — Y is never negative
// and never NaN, +inf (a sum that overflowed) lands in bin 255 like everything from 2^16 on.
PATCH_FN int pixelSlot( float r, float g, float b ) {
	const float Y = luminance( r, g, b );

	if( Y == 0.0f ) {
		return kDarkSlot;
	}

	const int bin = (int) ( floatBits( Y ) >> 20 ) - 888;
	return ( bin < 0 ) ? 0 : ( ( bin > 255 ) ? 255 : bin );
}

// One channel through exposure and curve, to [0, 1].  `white` is read by curve 1 only.
PATCH_FN float mapChannel( float c, float exposure, uint32_t curve, float white ) {
	const float x = clampTo( c * exposure, 65504.0f );
	float y = x;

	if( curve == PBR_DISPLAY_CURVE_REINHARD ) {
		y = ( x * ( 1.0f + x / ( white * white ) ) ) / ( 1.0f + x );
	}
	else if( curve == PBR_DISPLAY_CURVE_ACES ) {
		y = ( x * ( 2.51f * x + 0.03f ) ) / ( x * ( 2.43f * x + 0.59f ) + 0.14f );
	}

	return clampTo( y, 1.0f );
}

// pbr_read_display's arithmetic
PATCH_FN uint32_t encodeLinear( float y ) {
	return (uint32_t) (int) floorf( y * 255.0f + 0.5f );
}

// The number of k in 1 .. 255 with y >= T[k], T increasing: eight compare-and-select steps, no branch.  `T` is
// kSrgbThreshold or a copy of it (the map kernel's, in LDS).
PATCH_FN uint32_t encodeSrgb( const float* T, float y ) {
	uint32_t code = 0u;

	for( uint32_t step = 128u; step != 0u; step >>= 1 ) {
		code += ( y >= T[code + step] ) ? step : 0u;
	}

	return code;
}

PATCH_FN uint32_t encode( uint32_t transfer, const float* T, float y ) {
	return ( transfer == PBR_DISPLAY_TRANSFER_SRGB ) ? encodeSrgb( T, y ) : encodeLinear( y );
}

}   // namespace ptv

// ---- host only from here ----

// What pbr_display answers to these parameters before it touches the device.  Only the active mode's parameters are looked
// at, `white` only for curve 1; every message names the field.
inline int checkDisplayParams( const pbr_display_params* p, std::string* why ) {
	if( p == nullptr ) {
		return packFail( why, PBR_EINVAL, "pbr_display: null params" );
	}
	if( p->exposure_mode > PBR_DISPLAY_EXPOSURE_AUTO ) {
		return packFail( why, PBR_EINVAL, "pbr_display: exposure_mode %u (0 manual, 1 auto)", p->exposure_mode );
	}
	if( p->curve > PBR_DISPLAY_CURVE_ACES ) {
		return packFail( why, PBR_EINVAL, "pbr_display: curve %u (0 clamp, 1 extended Reinhard, 2 ACES fit)", p->curve );
	}
	if( p->transfer > PBR_DISPLAY_TRANSFER_SRGB ) {
		return packFail( why, PBR_EINVAL, "pbr_display: transfer %u (0 linear, 1 sRGB)", p->transfer );
	}

	if( p->exposure_mode == PBR_DISPLAY_EXPOSURE_MANUAL ) {
		if( !( std::isfinite( p->exposure ) && p->exposure > 0.0f ) ) {
			return packFail( why, PBR_EINVAL, "pbr_display: exposure %g (manual mode: finite and > 0)", (double) p->exposure );
		}
	}
	else {
		if( !( std::isfinite( p->key ) && p->key > 0.0f ) ) {
			return packFail( why, PBR_EINVAL, "pbr_display: key %g (auto mode: finite and > 0)", (double) p->key );
		}
		if( !( std::isfinite( p->low_fraction ) && p->low_fraction >= 0.0f ) ) {
			return packFail( why, PBR_EINVAL, "pbr_display: low_fraction %g (finite and >= 0)", (double) p->low_fraction );
		}
		if( !( std::isfinite( p->high_fraction ) && p->high_fraction >= 0.0f ) ) {
			return packFail( why, PBR_EINVAL, "pbr_display: high_fraction %g (finite and >= 0)", (double) p->high_fraction );
		}
		if( !( (double) p->low_fraction + (double) p->high_fraction < 1.0 ) ) {
			return packFail( why, PBR_EINVAL, "pbr_display: low_fraction %g + high_fraction %g leave nothing (their sum must be < 1)", (double) p->low_fraction, (double) p->high_fraction );
		}
		if( !( p->min_log2 >= -16.0f && p->min_log2 <= 16.0f ) ) {
			return packFail( why, PBR_EINVAL, "pbr_display: min_log2 %g (-16 <= min_log2 <= max_log2 <= 16)", (double) p->min_log2 );
		}
		if( !( p->max_log2 >= p->min_log2 && p->max_log2 <= 16.0f ) ) {
			return packFail( why, PBR_EINVAL, "pbr_display: max_log2 %g with min_log2 %g (-16 <= min_log2 <= max_log2 <= 16)", (double) p->max_log2, (double) p->min_log2 );
		}
		if( !( p->adapt > 0.0f && p->adapt <= 1.0f ) ) {
			return packFail( why, PBR_EINVAL, "pbr_display: adapt %g (in (0, 1]; 1 jumps to the target)", (double) p->adapt );
		}
	}

	if( p->curve == PBR_DISPLAY_CURVE_REINHARD && !( std::isfinite( p->white ) && p->white > 0.0f ) ) {
		return packFail( why, PBR_EINVAL, "pbr_display: white %g (curve 1: finite and > 0)", (double) p->white );
	}

	return PBR_OK;
}

// This image's target: the trimmed mean, in double, of the bin centres over the 256 counts, clamped.  *counted = N.  With
// N == 0 the remembered value if there is one, else 0.  Additions, multiplications and divisions in this order only.
inline double displayTarget( const uint32_t counts[256], const pbr_display_params& p, bool remembered, double previous, uint64_t* counted ) {
	uint64_t total = 0;

	for( int b = 0; b < ptv::kBins; b++ ) {
		total += counts[b];
	}

	*counted = total;

	if( total == 0 ) {
		return remembered ? previous : 0.0;
	}

	const double N = (double) total;
	const double lo = (double) p.low_fraction * N;
	const double hi = N - (double) p.high_fraction * N;
	double below = 0.0, weighted = 0.0, kept = 0.0;

	for( int b = 0; b < ptv::kBins; b++ ) {
		const double upTo = below + (double) counts[b];
		const double top = ( upTo < hi ) ? upTo : hi;
		const double bottom = ( below > lo ) ? below : lo;
		const double share = ( top - bottom > 0.0 ) ? top - bottom : 0.0;
		weighted = weighted + share * ( ( (double) b + 0.5 ) / 8.0 - 16.0 );
		kept = kept + share;
		below = upTo;
	}

	const double m = weighted / kept;
	const double lowest = (double) p.min_log2, highest = (double) p.max_log2;
	return ( m < lowest ) ? lowest : ( ( m > highest ) ? highest : m );
}

// Where the exposure goes from `previous` towards `target` in one call.
inline double displayAdapt( double target, const pbr_display_params& p, bool remembered, double previous ) {
	if( !remembered || p.adapt == 1.0f ) {
		return target;
	}

	return previous + (double) p.adapt * ( target - previous );
}

inline float displayExposure( const pbr_display_params& p, double log2Used ) {
	return (float) ( (double) p.key * std::exp2( -log2Used ) );
}
