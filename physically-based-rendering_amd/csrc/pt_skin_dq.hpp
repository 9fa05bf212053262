// pt_skin_dq.hpp — the kernels pbr_update_skin_dq and pbr_update_pose_dq put in front of the refit's (pt_refit.hpp,
// pt_patch_refit.hpp; host side: pbr_hip.hip).  All four stream: one thread per vertex / per normal, 256 per workgroup, one
// 16-byte load of the rest quad, two 16-byte loads of the element's influence record (pts::Influence, read with pt_skin.hpp's
// loadInfluence), two 16-byte loads of a 32-byte bone record — the real and the dual quad — per slot whose weight is not 0, one
// 16-byte store: 64 bytes of unavoidable traffic per element, 32 per active slot on top (the matrix skin reads 48).  The pose
// kernels add the run words and the entries exactly as poseVertices reads them (pt_morph.hpp).
//
//   skinVerticesDQ  V' = dq skin( rest ) into the skin's STAGING buffer (pt_skin_dq_host.hpp, ptq::skinPositionDQ: the same source
//                   the host unit is built from).  A position with a word that is not finite raises *flag — once per wave: a
//                   ballot, then the first lane that saw one stores a 1 (plain store; every writer stores the same word),
//                   exactly as skinVertices does.  The host reads the flag before the staging buffer becomes the context's
//                   vertices.
//   skinNormalsDQ   N' = unit( rest turned by the element's blend ) straight into the patch refit's normal table; it cannot fail.
//   poseVerticesDQ  V' = dq skin( morph( rest ) ) into the morph's staging buffer, flagged the same way.
//   poseNormalsDQ   N' = dq skin( morph( rest ) ) for a morph with normal targets under a skin with normal influences.  (A pose
//                   whose morph has no normal targets launches skinNormalsDQ, one whose skin has no normal influences
//                   morphNormals.)
//
// Per element the arithmetic is about 120 flops, one square root and eight divisions, both correctly rounded — small next to the
// bytes moved; the bone records are not staged in LDS, on pt_skin.hpp's argument (a 32-byte record, neighbours mostly share
// their bones).  The bone table is skin.dBones, 48 bytes per bone allocated, 32 used.  No workgroup talks to another; nothing
// here is shared between lanes but the ballot.
//
// Bounds: the host has checked every bone index against the bone count before the influence records were uploaded (checkSkin:
// zero-weight slots too), `influences` holds two quads per element and `bones` two per bone; the pose kernels' runs are
// packMorph's (runFirst[count + 1], every target < num_targets).
#pragma once

#include <hip/hip_runtime.h>

#include "pt_morph.hpp"
#include "pt_skin_dq_host.hpp"

namespace ptr {

__global__ __launch_bounds__( 256 ) void skinVerticesDQ( const float4* __restrict__ rest, const uint4* __restrict__ influences,
                                                         const float4* __restrict__ bones, float4* __restrict__ staged,
                                                         unsigned* __restrict__ flag, int numVertices ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );
	bool bad = false;

	if( i < numVertices ) {
		uint32_t slots[4];
		float weights[4];
		const float4 p = rest[i];
		loadInfluence( influences, i, slots, weights );
		const float4 moved = ptq::skinPositionDQ( bones, slots, weights, p );
		bad = !ptx::finitePosition( moved );
		staged[i] = moved;
	}

	raiseOncePerWave( bad, flag );
}

__global__ __launch_bounds__( 256 ) void skinNormalsDQ( const float4* __restrict__ rest, const uint4* __restrict__ influences,
                                                        const float4* __restrict__ bones, float4* __restrict__ normals, int numNormals ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( i >= numNormals ) {
		return;
	}

	uint32_t slots[4];
	float weights[4];
	const float4 n = rest[i];
	loadInfluence( influences, i, slots, weights );
	normals[i] = ptq::skinNormalDQ( bones, slots, weights, n );
}

__global__ __launch_bounds__( 256 ) void poseVerticesDQ( const float4* __restrict__ rest, const uint32_t* __restrict__ runFirst,
                                                         const ptm::Entry* __restrict__ entries, const float* __restrict__ weights,
                                                         const uint4* __restrict__ influences, const float4* __restrict__ bones,
                                                         float4* __restrict__ staged, unsigned* __restrict__ flag, int numVertices ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );
	bool bad = false;

	if( i < numVertices ) {
		uint32_t slots[4];
		float blend[4];
		loadInfluence( influences, i, slots, blend );
		const float4 moved = ptq::posePositionDQ( entries, runFirst[i], runFirst[i + 1], weights, bones, slots, blend, rest[i] );
		bad = !ptx::finitePosition( moved );
		staged[i] = moved;
	}

	raiseOncePerWave( bad, flag );
}

__global__ __launch_bounds__( 256 ) void poseNormalsDQ( const float4* __restrict__ rest, const uint32_t* __restrict__ runFirst,
                                                        const ptm::Entry* __restrict__ entries, const float* __restrict__ weights,
                                                        const uint4* __restrict__ influences, const float4* __restrict__ bones,
                                                        float4* __restrict__ normals, int numNormals ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( i >= numNormals ) {
		return;
	}

	uint32_t slots[4];
	float blend[4];
	loadInfluence( influences, i, slots, blend );
	normals[i] = ptq::poseNormalDQ( entries, runFirst[i], runFirst[i + 1], weights, bones, slots, blend, rest[i] );
}

}   // namespace ptr
