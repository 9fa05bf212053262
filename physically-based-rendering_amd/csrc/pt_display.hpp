// pt_display.hpp — the two kernels of pbr_display (host side: pbr_hip.hip; the per-pixel arithmetic: pt_display_host.hpp, the
// same source the host unit is built from).  Every output is reproducible to the bit: the histogram's adds are integer adds,
// the map has no cross-lane arithmetic at all.
//
//   displayHistogram  a stream of `groups` groups of 64 pixels — the 8 x 8 tiles of the tile-major framebuffer, or 64 neighbours
//                     of a row-major host image: a count does not care — one group per wave and trip of a grid-stride loop,
//                     one 16-byte load per pixel, 1 KiB contiguous per wave.  Counts go into LDS first, one sub-histogram PER
//                     WAVE (4 x 257 words), so that no two waves ever meet on a word; then the workgroup adds its four
//                     sub-histograms and flushes the slots that are not zero with one relaxed, agent-scope vector atomic
//                     each into `counts`, which the call has zeroed on the stream.  Slot 256 counts the pixels with Y == 0.
//                     The grid is bounded (kHistogramMaxBlocks): a 4K frame costs 2048 x 257 far atomics at the most.
//                     Rendered images put most pixels of a wave into a handful of bins, and 64 LDS atomics on one word are
//                     served one after the other.  MERGE rounds take that out: per round the first lane that still holds a
//                     pixel names its slot, a ballot counts the lanes that hold the same, that lane adds the count once and
//                     all of them retire; what is left after the rounds adds 1 per lane.  An all-equal wave costs one LDS add
//                     instead of 64; a wave of 64 different slots pays MERGE ballots for nothing.  MERGE is chosen by
//                     measurement (the "display_merge" knob picks another build for such a run).
//   displayMap        one thread per output pixel, 64 x 4 blocks as every image kernel here: one 16-byte load (tile-major with
//                     the dealing of a sharded context, or row-major), exposure, curve and encode per channel, one 4-byte
//                     store, contiguous along a row.  The sRGB table is staged in LDS once per workgroup (1 KiB; the search
//                     reads eight words of it per channel, lanes at different words: LDS serves that, the scalar cache would
//                     not).  The linear transfer stages nothing.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_display_host.hpp"
#include "pt_kernel.hpp"

namespace ptv {

const unsigned kHistogramBlock = 256u;          // four waves, a sub-histogram each
const unsigned kHistogramMaxBlocks = 2048u;     // one trip of the stride loop covers 8192 groups = 524288 pixels

inline unsigned histogramBlocks( size_t groups ) {
	const size_t wanted = ( groups + 3u ) / 4u;
	return (unsigned) ( wanted < kHistogramMaxBlocks ? ( wanted > 0 ? wanted : 1 ) : kHistogramMaxBlocks );
}

template<int MERGE>
__global__ __launch_bounds__( 256 ) void displayHistogram( const float4* __restrict__ pixels, unsigned groups, unsigned* __restrict__ counts ) {
	__shared__ unsigned sub[4][kCountSlots];
	const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;

	for( unsigned i = threadIdx.x; i < 4u * kCountSlots; i += kHistogramBlock ) {
		( &sub[0][0] )[i] = 0u;
	}

	__syncthreads();

	// wave-uniform bounds: all 64 lanes of a wave run every trip together
	for( unsigned group = blockIdx.x * 4u + wave; group < groups; group += gridDim.x * 4u ) {
		const float4 v = pixels[(size_t) group * 64u + lane];
		const int slot = pixelSlot( v.x, v.y, v.z );
		bool pending = true;

		for( int round = 0; round < MERGE; round++ ) {
			const unsigned long long waiting = __ballot( pending );

			if( waiting == 0ull ) {
				break;
			}

			const int leader = __ffsll( (long long) waiting ) - 1;
			const int named = __shfl( slot, leader, 64 );
			const bool same = pending && slot == named;
			const unsigned long long merged = __ballot( same );

			if( (int) lane == leader ) {
				atomicAdd( &sub[wave][named], (unsigned) __popcll( merged ) );
			}

			pending = pending && !same;
		}

		if( pending ) {
			atomicAdd( &sub[wave][slot], 1u );
		}
	}

	__syncthreads();

	for( unsigned i = threadIdx.x; i < (unsigned) kCountSlots; i += kHistogramBlock ) {
		const unsigned total = ( sub[0][i] + sub[1][i] ) + ( sub[2][i] + sub[3][i] );

		if( total != 0u ) {
			__hip_atomic_fetch_add( counts + i, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
		}
	}
}

// What the map kernel is told: the exposure the host found or was given, the curve and transfer, and where the pixels are.
struct MapArgs {
	float exposure, white;
	unsigned curve, transfer;
	int width, height;
	int rowMajor;               // 1: `src` is width x height, row 0 = bottom; 0: tile-major local tiles, dealt as below
	int tilesX, tileWorld, tileRank;
	int topRowFirst;
};

__global__ __launch_bounds__( 256 ) void displayMap( const float4* __restrict__ src, const float* __restrict__ table, uchar4* __restrict__ rows, const MapArgs A ) {
	__shared__ float T[256];

	if( A.transfer == PBR_DISPLAY_TRANSFER_SRGB ) {
		const unsigned t = threadIdx.y * 64u + threadIdx.x;
		T[t] = table[t];
	}

	__syncthreads();
	const int x = (int) ( blockIdx.x * blockDim.x + threadIdx.x );
	const int y = (int) ( blockIdx.y * blockDim.y + threadIdx.y );

	if( x >= A.width || y >= A.height ) {
		return;
	}

	float4 v = make_float4( 0.0f, 0.0f, 0.0f, 0.0f );

	if( A.rowMajor ) {
		v = src[(size_t) y * (size_t) A.width + (size_t) x];
	}
	else {
		const int position = ptk::dealPositionOfTile( ( y >> 3 ) * A.tilesX + ( x >> 3 ), A.tilesX, A.tileWorld );

		if( position % A.tileWorld == A.tileRank ) {
			v = src[(size_t) ( position / A.tileWorld ) * 64 + (size_t) ( ( y & 7 ) * 8 + ( x & 7 ) )];
		}
	}

	const unsigned r = encode( A.transfer, T, mapChannel( v.x, A.exposure, A.curve, A.white ) );
	const unsigned g = encode( A.transfer, T, mapChannel( v.y, A.exposure, A.curve, A.white ) );
	const unsigned b = encode( A.transfer, T, mapChannel( v.z, A.exposure, A.curve, A.white ) );
	const int outRow = A.topRowFirst ? ( A.height - 1 - y ) : y;
	rows[(size_t) outRow * (size_t) A.width + (size_t) x] = make_uchar4( (unsigned char) r, (unsigned char) g, (unsigned char) b, 255 );
}

}   // namespace ptv
