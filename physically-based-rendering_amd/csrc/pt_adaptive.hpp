// pt_adaptive.hpp — the fold of an adaptive render (pbr_render_adaptive; host side: pbr_hip.hip launchAdaptive,
// pt_adaptive_host.hpp).  Included by pbr_hip.hip only, next to pt_aux.hpp; exists once (no build flavour: it reads the frame
// buffer, whatever arithmetic filled it).
//
// foldFramesAdaptive is foldFrames for the tiles a round rendered — the same running mean by the same expressions, the image
// bits depend on it — plus the error estimate that stops a tile.  ONE WAVE PER ACTIVE TILE, lane = pixel slot of the tile.
//
// The estimate is fixed operation by operation in binary32 (the library is built -ffp-contract=off and with correctly rounded
// divisions and square roots; there is no fma in it), so that tests/adaptive_ref.py reproduces its bits — and so the stop
// decisions — with numpy float32:
//   per pixel slot, over the frames of the call in frame order (k counts them from 1), with Y = ( 0.2126 r + 0.7152 g ) + 0.0722 b
//   of the frame's colour:   d = Y - mean ;  mean = mean + d / k ;  M2 = M2 + d * ( Y - mean )          (Welford)
//   per tile at a round end with c frames:   v = M2 / ( c - 1 ) / c   per lane (the variance of the pixel's mean),
//   V = sum of v, S = sum of mean over the 64 lanes by the xor butterfly x += shfl_xor( x, step ), step = 32, 16 ... 1
//   (commutative additions: every lane ends with the same bits),
//   error = sqrt( V / 64 ) / ( S / 64 + 0.01 )   — the relative standard error of the tile's mean luminance; the 0.01 keeps
//   black tiles finite.  The tile stops when error <= threshold; a NaN (a frame that is not finite) compares false and
//   keeps the tile active.
// Bound by HBM: 16 B per pixel and frame + 32 B per pixel (image in, image out) + 16 B per pixel for the moments; the
// reduction is 2 x 6 cross-lane steps per tile and round.  No LDS, no scratch.
#pragma once

#include "pt_kernel.hpp"

namespace ptk {

// tiles[0 .. numActive): the local tiles this launch pair rendered (the round's dealing table: it names each of them once).
// src / dst: the running mean before / after (the input image for the call's first pair, imageOut after it); tiles that are
// not listed are not touched.  framesBefore: frames of this call the listed tiles had before this pair (0: the moments start
// at 0, the table is not read).  roundEnd: test the tiles — tileFrames / tileError / tileActive [tile] are written then.
__global__ __launch_bounds__( 256 ) void foldFramesAdaptive( const DevParams P, const float4* src, float4* dst, const unsigned* tiles, unsigned numActive,
                                                             float2* moments, unsigned framesBefore, int roundEnd, float threshold,
                                                             unsigned* tileFrames, float* tileError, unsigned* tileActive ) {
	const unsigned thread = blockIdx.x * blockDim.x + threadIdx.x;

	// as foldFrames: the path-tracing launch before this one has drained the queue — leave its heads (and the word of the
	// heads seen empty behind them) at zero for the next launch (the grid has at least one block of 256 threads)
	if( thread <= (unsigned) PT_HEADS ) {
		P.workCounter[thread * PT_BAND_STRIDE] = 0u;
	}

	const unsigned listed = thread >> 6;

	if( listed >= numActive ) {
		return;
	}

	const unsigned tile = tiles[listed];

	if( tile >= (unsigned) P.numLocalTiles ) {   // (a table the host filtered names local tiles only: never true)
		return;
	}

	const unsigned slot = tile * 64u + ( threadIdx.x & 63u );
	float4 acc = src[slot];
	float2 m = make_float2( 0.0f, 0.0f );   // {mean, M2} of the luminance

	if( framesBefore != 0u ) {
		m = moments[slot];
	}

	for( int k = 0; k < P.nFrames; k++ ) {
		const float4 fc = P.frameBuf[frameBufIndex( P, slot, (unsigned) k )];
		// setColors, literally as foldFrames has it
		const unsigned n = (unsigned) ( P.firstCount + k );
		const float w = (float) n / (float) ( n + 1u );
		acc.x = fc.x + ( acc.x - fc.x ) * w;
		acc.y = fc.y + ( acc.y - fc.y ) * w;
		acc.z = fc.z + ( acc.z - fc.z ) * w;
		acc.w = fc.w;

		const float y = ( 0.2126f * fc.x + 0.7152f * fc.y ) + 0.0722f * fc.z;
		const float count = (float) ( framesBefore + (unsigned) k + 1u );
		const float d = y - m.x;
		m.x = m.x + d / count;
		m.y = m.y + d * ( y - m.x );
	}

	dst[slot] = acc;
	moments[slot] = m;

	if( !roundEnd ) {
		return;
	}

	const unsigned c = framesBefore + (unsigned) P.nFrames;
	float v = m.y / (float) ( c - 1u ) / (float) c;
	float s = m.x;

	for( int step = 32; step >= 1; step >>= 1 ) {
		v += __shfl_xor( v, step, 64 );
		s += __shfl_xor( s, step, 64 );
	}

	const float error = sqrtf( v / 64.0f ) / ( s / 64.0f + 0.01f );

	if( ( threadIdx.x & 63u ) == 0u ) {
		tileFrames[tile] = c;
		tileError[tile] = error;
		tileActive[tile] = ( error <= threshold ) ? 0u : 1u;
	}
}

}  // namespace ptk
