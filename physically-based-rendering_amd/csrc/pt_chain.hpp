// The focus chain: what a multi-frame render with depth of field needs from one frame to the next (pbr_render_dof).
//
// Frame k of a pixel p reads two values of frame k - 1 (focusInputs, pt_kernel.hpp): .w of its own pixel and .w of the focus
// pixel — and .w of a frame is the distance of the first hit of its first sample's camera ray (shadeStep).  So between the
// frames of a launch runs a chain of camera-ray first hits per pixel and nothing else of a path,
//
//     t_k( p ) = firstHit( initRay( p, seeds[k], tFocus = t_{k-1}( focus pixel ), tObject = t_{k-1}( p ) ) ),   t_{-1} = imageIn.w
//
// Two kernels compute it ahead of the frame-parallel launch, which then finds the inputs of every (pixel, frame) unit in
// P.chain and runs as it does without a focus point:
//
//   focusChainPixel   one lane walks the focus pixel's n camera rays one after the other.  Every rank of a sharded render
//                     does this itself (the scene is replicated), from the distance pbr_set_focus_depth handed it once.
//   focusChainSlots   one lane per local pixel slot — a wave is one 8 x 8 tile: coherent rays, one coalesced KiB of the
//                     previous image — looping over the frames.
//
// Both call initRay and traverse of THIS build flavour's namespace (pt_flavour.hpp; pt_instance.hip, group PTI_CHAIN): the
// walk order and the arithmetic are the path kernels', so the bits are theirs.  The walks are not counted: the counters, the
// debug image and the tile costs learnt from it stay those of the paths.  The node phase is traverse()'s C++ loop on the
// stream in memory (no staged prefix: a launch this short does not earn the staging), whose trips PBR_GUARD builds bound;
// the frame loops here are counted loops.
#pragma once

#include "pt_kernel.hpp"

namespace ptk {

// t_k of one pixel from t_{k-1}: the first sample's camera ray of frame k and its closest hit (a miss, or an orb light, is inf)
template<bool LIGHTS>
PT_DEV float chainStep( const DevParams& P, int px, int py, unsigned k, float tFocus, float tObject ) {
	float seed = P.seeds[k];
	const Ray ray = initRay( P, px, py, seed, tFocus, tObject );
	Hit hit;
	hit.t = inff();
	hit.face = 0;
	hit.normal = mk3( 0.0f, 0.0f, 0.0f );
	unsigned nodes = 0, tris = 0;
	traverse<false, LIGHTS, false>( P, nullptr, ray, hit, nodes, tris );
	return hit.t;
}

// prev: the image before the first frame of this launch.  The start value is prev.w of the focus pixel (CLAMP_TO_EDGE, as
// focusInputs reads it) — or, with tile sharding (P.focusGiven), what the caller handed over: P.focusDepth for the first
// launch of a render, *carry (this kernel's own last value) for the launches after it.
template<bool LIGHTS>
__global__ __launch_bounds__( 64 ) void focusChainPixel( const DevParams P, const float4* prev, float* chain, float* carry, int useCarry ) {
	if( blockIdx.x != 0 || threadIdx.x != 0 ) {
		return;
	}

	const int fx = ( P.focusX > P.width - 1 ) ? P.width - 1 : P.focusX;
	const int fy = ( P.focusY > P.height - 1 ) ? P.height - 1 : P.focusY;
	float tFocus, tObject;

	if( P.focusGiven ) {
		tFocus = useCarry ? *carry : P.focusDepth;
		tObject = tFocus;
	}
	else {
		const int ft = ( fy >> 3 ) * P.tilesX + ( fx >> 3 );
		tFocus = prev[(size_t) ft * 64 + (size_t) ( ( fy & 7 ) * 8 + ( fx & 7 ) )].w;
		tObject = tFocus;
	}

	// an unsharded context that was handed a distance all the same: the focus pixel's own previous value is still its own
	if( P.focusGiven && !useCarry && P.tileWorld <= 1 ) {
		const int ft = ( fy >> 3 ) * P.tilesX + ( fx >> 3 );
		tObject = prev[(size_t) ft * 64 + (size_t) ( ( fy & 7 ) * 8 + ( fx & 7 ) )].w;
	}

	for( unsigned k = 0; k < (unsigned) P.nFrames; k++ ) {
		chain[P.chainFocusAt + k] = tFocus;
		tFocus = chainStep<LIGHTS>( P, fx, fy, k, tFocus, tObject );
		tObject = tFocus;
	}

	*carry = tFocus;
}

// after focusChainPixel: chain[chainFocusAt + k] is there for every frame of the launch
template<bool LIGHTS>
__global__ __launch_bounds__( 256 ) void focusChainSlots( const DevParams P, const float4* prev, float* chain ) {
	const unsigned slot = blockIdx.x * blockDim.x + threadIdx.x;

	if( slot >= P.frameStride ) {   // whole waves: the slots are a multiple of 64
		return;
	}

	int px, py;
	pixelOfSlot( P, slot, &px, &py );
	float t = prev[slot].w;

	for( unsigned k = 0; k < (unsigned) P.nFrames; k++ ) {
		chain[slot * P.chainSlotStride + k * P.chainFrameStride] = t;
		t = chainStep<LIGHTS>( P, px, py, k, chain[P.chainFocusAt + k], t );
	}
}

}  // namespace ptk
