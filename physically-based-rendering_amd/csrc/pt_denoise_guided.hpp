// pt_denoise_guided.hpp — the variance of an adaptive render's pixels and the filter it guides (pbr_read_variance,
// pbr_denoise_guided; host side: pbr_hip.hip).  Included by pbr_hip.hip only, behind pt_denoise.hpp; exists once (no build
// flavour: it reads the accumulated image and the moments, whatever arithmetic filled them).
//
// pbr_render_adaptive keeps, per pixel slot, Welford's {mean, M2} of the luminance over the frames of the call
// (pt_adaptive.hpp) and per tile the frames it rendered.  `pixelVariance` turns them into the variance of the pixel's MEAN:
//   var = M2 / (float) ( c - 1 ) / (float) ( n0 + c ),   c the tile's frames, n0 the call's first_sample_count
// — two binary32 divisions in that order (the library is built -ffp-contract=off with correctly rounded divisions and
// square roots), so tests/guided_denoise_ref.py reproduces its bits.  For n0 = 0 it is the `v` of foldFramesAdaptive.
//
// `atrousGuidedPass` is atrousPass (pt_denoise.hpp) with two differences — SVGF's spatial part (Schied et al. 2017) without
// its temporal part: the colour term is replaced by a luminance term in units of the LOCAL standard deviation, and the
// variance is filtered along with the colour.  Pass k, step s = 2^k, on colour C and variance V (C_0 the accumulated image,
// V_0 = var), for the pixel p:
//   1. g = sum of G_i G_j V( p + (i, j) ) / sum of G_i G_j over |i|, |j| <= 1, G = {0.25, 0.5, 0.25}, taps ONE pixel apart
//      whatever s is; taps outside the image or whose V is not finite are left out, g = 0 if none is left; sd = sqrt( g )
//   2. e_l = | Y( C( q ) ) - Y( C( p ) ) | / ( sigma_luminance * sd + 1e-6 ), Y = ( 0.2126 r + 0.7152 g ) + 0.0722 b;
//      sigma_luminance = 0: e_l = 0
//   3. e = e_l, and for a hit centre + the normal, world and albedo terms of atrousPass, in that order
//   4. the 5 x 5 taps q, s pixels apart, j outer, i inner; skipped: outside the image, across the hit / miss divide,
//      !( e < inf ), V( q ) not finite;  w = ( spline_i * spline_j ) * expf( -e )
//   5. C'( p ) = sum w C( q ) / sum w;  V'( p ) = sum ( w * w ) V( q ) / ( sum w * sum w );  both stay if sum w is not in (0, inf)
// With sigma_luminance = 0 the colour is bit for bit atrousPass's with sigma_color = 0: same taps, same order, same
// accumulation expressions, same expf.
//
// One thread per pixel, 64 x 4 blocks, no LDS: at steps 4 .. 16 the halo exceeds the tile.  atrousPass never reads a tap's
// .w, so in the working buffers the variance rides there: no extra load per tap, and the nine taps of step 1 read the same
// buffer (neighbouring lanes' lines).  The last pass puts the accumulated first-hit distance back from the untiled original.
#pragma once

#include "pt_denoise.hpp"

namespace ptd {

__device__ __forceinline__ float luminance( float4 c ) {
	return ( 0.2126f * c.x + 0.7152f * c.y ) + 0.0722f * c.z;
}

__device__ __forceinline__ bool finite1( float x ) {
	return fabsf( x ) < inff();   // false for NaN
}

// moments / tileFrames: of the local tiles (tile_world = 1: every tile, at its dealing position).  variance (may be null):
// W x H floats, row-major.  working (may be null): rows' colour with the variance in .w — the filter's first input.
__global__ void pixelVariance( const float2* moments, const unsigned* tileFrames, unsigned firstCount, const float4* rows,
                               float* variance, float4* working, int width, int height, int tilesX ) {
	const int x = (int) ( blockIdx.x * blockDim.x + threadIdx.x );
	const int y = (int) ( blockIdx.y * blockDim.y + threadIdx.y );

	if( x >= width || y >= height ) {
		return;
	}

	// untile's addressing (pt_aux.hpp) for an unsharded context
	const int tileGlobal = ( y >> 3 ) * tilesX + ( x >> 3 );
	const int tileLocal = ptk::dealPositionOfTile( tileGlobal, tilesX, 1 );
	const unsigned c = tileFrames[tileLocal];
	const float m2 = moments[(size_t) tileLocal * 64 + (size_t) ( ( y & 7 ) * 8 + ( x & 7 ) )].y;
	const float var = m2 / (float) ( c - 1u ) / (float) ( firstCount + c );
	const size_t at = (size_t) y * (size_t) width + (size_t) x;

	if( variance != nullptr ) {
		variance[at] = var;
	}
	if( working != nullptr ) {
		const float4 v = rows[at];
		working[at] = make_float4( v.x, v.y, v.z, var );
	}
}

// in / out: {colour, variance}.  original / varianceOut: null but in the last pass, which writes {colour, original .w} and
// the variance on its own.
__global__ void atrousGuidedPass( const GuidedArgs A, const float4* in, float4* out, const float4* position, const float4* normal, const float4* albedo,
                                  const float4* original, float* varianceOut ) {
	const int x = (int) ( blockIdx.x * blockDim.x + threadIdx.x );
	const int y = (int) ( blockIdx.y * blockDim.y + threadIdx.y );

	if( x >= A.width || y >= A.height ) {
		return;
	}

	const float spline[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
	const float gauss[3] = { 0.25f, 0.5f, 0.25f };
	const size_t at = (size_t) y * (size_t) A.width + (size_t) x;
	const float4 c0 = in[at], p0 = position[at], n0 = normal[at], a0 = albedo[at];
	const float sigmaWorld = A.worldScale * p0.w;
	const float invWorld = ( n0.w != 0.0f && sigmaWorld > 0.0f ) ? 1.0f / ( sigmaWorld * sigmaWorld ) : 0.0f;

	// 1. the local variance: 3 x 3 taps one pixel apart
	float sumGV = 0.0f, sumG = 0.0f;

	for( int j = -1; j <= 1; j++ ) {
		const int ty = y + j;

		if( ty < 0 || ty >= A.height ) {
			continue;
		}

		for( int i = -1; i <= 1; i++ ) {
			const int tx = x + i;

			if( tx < 0 || tx >= A.width ) {
				continue;
			}

			const float v = in[(size_t) ty * (size_t) A.width + (size_t) tx].w;

			if( !finite1( v ) ) {
				continue;
			}

			const float g = gauss[i + 1] * gauss[j + 1];
			sumGV += g * v;
			sumG += g;
		}
	}

	const float local = ( sumG > 0.0f ) ? sumGV / sumG : 0.0f;
	const float scale = A.sigmaLuminance * sqrtf( local ) + 1e-6f;
	const float y0 = luminance( c0 );
	float sumR = 0.0f, sumG2 = 0.0f, sumB = 0.0f, sumW = 0.0f, sumV = 0.0f;

	for( int j = -2; j <= 2; j++ ) {
		const int ty = y + j * A.step;

		if( ty < 0 || ty >= A.height ) {
			continue;
		}

		for( int i = -2; i <= 2; i++ ) {
			const int tx = x + i * A.step;

			if( tx < 0 || tx >= A.width ) {
				continue;
			}

			const size_t tap = (size_t) ty * (size_t) A.width + (size_t) tx;
			const float4 n = normal[tap];

			if( n.w != n0.w ) {
				continue;
			}

			const float4 c = in[tap];
			float e = 0.0f;

			if( A.sigmaLuminance != 0.0f ) {
				e = fabsf( luminance( c ) - y0 ) / scale;
			}

			if( n0.w != 0.0f ) {
				e += squaredDistance3( n, n0 ) * A.invNormal;
				e += squaredDistance3( position[tap], p0 ) * invWorld;
				e += squaredDistance3( albedo[tap], a0 ) * A.invAlbedo;
			}

			if( !( e < inff() ) || !finite1( c.w ) ) {
				continue;   // a tap that is not finite (or infinitely far in some feature), or whose variance is not, has no say
			}

			const float w = ( spline[i + 2] * spline[j + 2] ) * expf( -e );
			sumR += w * c.x;
			sumG2 += w * c.y;
			sumB += w * c.z;
			sumW += w;
			sumV += ( w * w ) * c.w;
		}
	}

	const bool usable = sumW > 0.0f && sumW < inff();
	float4 result = usable ? make_float4( sumR / sumW, sumG2 / sumW, sumB / sumW, sumV / ( sumW * sumW ) ) : c0;

	if( varianceOut != nullptr ) {
		varianceOut[at] = result.w;
	}
	if( original != nullptr ) {
		result.w = original[at].w;
	}

	out[at] = result;
}

}  // namespace ptd
