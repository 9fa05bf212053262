// pt_morph.hpp — the kernels pbr_update_morph and pbr_update_pose put in front of the refit's (pt_refit.hpp, pt_patch_refit.hpp;
// host side: pbr_hip.hip).  All four stream: one thread per vertex / per normal, 256 per workgroup, one 16-byte load of the rest
// quad, the two runFirst words of the element, per entry of its run one 16-byte load ( dx, dy, dz, target ) and one read of
// weights[target], one 16-byte store — 40 bytes of unavoidable traffic per element, 16 per entry on top; the weight table is
// num_targets floats and stays in the scalar / vector caches.  The pose kernels add the influence record and the bone records
// exactly as skinVertices reads them (pt_skin.hpp).
//
//   morphVertices  V' = morph( rest ) into the morph's STAGING buffer (pt_morph_host.hpp, ptm::morphPosition: the same source the
//                  host unit is built from).  A position with a word that is not finite raises *flag — once per wave: a ballot,
//                  then the first lane that saw one stores a 1 (plain store; every writer stores the same word), exactly as
//                  skinVertices does.  The host reads the flag before the staging buffer becomes the context's vertices.
//   morphNormals   N' = unit( rest + sum w d ) straight into the patch refit's normal table; it cannot fail.
//   poseVertices   V' = skin( morph( rest ) ), staged and flagged like morphVertices.
//   poseNormals    N' = skin( morph( rest ) ) for a morph with normal targets under a skin with normal influences.  (A pose whose
//                  morph has no normal targets launches skinNormals, one whose skin has no normal influences morphNormals.)
//
// THE RUNS VARY IN LENGTH, which is where these kernels differ from their siblings: a wave's cost is its longest run, and sparse
// targets leave most lanes with a run of 0.  This is the plain one-thread-per-element loop; the entries of one element are
// contiguous (packMorph), so a lane walks 16-byte steps through its own run and neighbouring lanes' runs are adjacent in memory.
// 17 / 19 VGPRs (morph), 40 / 38 (pose), no spill, 8 waves per SIMD.
//
// Measured (profiles/r17/experiments/morph.txt; BASELINE scenes, medians of 9, kernels' bytes over their time):
//   8 or 64 targets of 5 % each (runs of 0 .. 10, 0.4 or 3.2 on average)   0.014 – 0.139 ms, 830 – 4270 GB/s: the skin kernels'
//                                                                           rate in the same run (1150 – 3560 GB/s) or above it
//   64 targets naming every element (every run is 64)                       0.234 / 1.640 / 7.858 ms, 1207 / 562 / 540 GB/s —
//                                                                           a sixth of the skin kernels' rate on the two larger
//                                                                           scenes
// In the dense case every run has the same length, so the imbalance between the lanes of a wave is NOT what costs there.  What
// the loop does is this: in step k lane i reads entry runFirst[i] + k, and with runs of 64 neighbouring lanes are 1 KiB apart —
// one load instruction touches 64 cache lines for 1 KiB of use, and a line is fetched for eight steps of one lane; eight waves
// per SIMD keep more lines in flight than a CU's vector L1 holds.  That is the suspected cause (not isolated by a counter run).
// With sparse targets most lanes have nothing to read and the rest quads' and the stores' coalesced traffic dominates.  A
// wave-cooperative variant — the wave walks its 64 elements' concatenated runs, one entry per lane, consecutive addresses, and
// reduces per element in target order — would address both the stride and the imbalance; it has to keep the order of the
// additions to stay bit-identical.  It is a follow-up and not built.  No workgroup talks to another, there is no atomic and no
// LDS here.
//
// Bounds: the host has checked every element index against the upload's count and packMorph wrote runFirst[count + 1] with
// runFirst[count] = the number of entries, every entry's target < num_targets (checkMorph, packMorph); the pose kernels' bone
// indices are checkSkin's.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_morph_host.hpp"
#include "pt_skin.hpp"

namespace ptr {

__device__ inline void raiseOncePerWave( bool bad, unsigned* __restrict__ flag ) {
	const unsigned long long raised = __ballot( bad );

	if( bad && ( raised & ( ( 1ull << ( threadIdx.x & 63u ) ) - 1ull ) ) == 0ull ) {
		*flag = 1u;
	}
}

__global__ __launch_bounds__( 256 ) void morphVertices( const float4* __restrict__ rest, const uint32_t* __restrict__ runFirst,
                                                        const ptm::Entry* __restrict__ entries, const float* __restrict__ weights,
                                                        float4* __restrict__ staged, unsigned* __restrict__ flag, int numVertices ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );
	bool bad = false;

	if( i < numVertices ) {
		const float4 moved = ptm::morphPosition( entries, runFirst[i], runFirst[i + 1], weights, rest[i] );
		bad = !ptx::finitePosition( moved );
		staged[i] = moved;
	}

	raiseOncePerWave( bad, flag );
}

__global__ __launch_bounds__( 256 ) void morphNormals( const float4* __restrict__ rest, const uint32_t* __restrict__ runFirst,
                                                       const ptm::Entry* __restrict__ entries, const float* __restrict__ weights,
                                                       float4* __restrict__ normals, int numNormals ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( i >= numNormals ) {
		return;
	}

	normals[i] = ptm::morphNormal( entries, runFirst[i], runFirst[i + 1], weights, rest[i] );
}

__global__ __launch_bounds__( 256 ) void poseVertices( const float4* __restrict__ rest, const uint32_t* __restrict__ runFirst,
                                                       const ptm::Entry* __restrict__ entries, const float* __restrict__ weights,
                                                       const uint4* __restrict__ influences, const float4* __restrict__ bones,
                                                       float4* __restrict__ staged, unsigned* __restrict__ flag, int numVertices ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );
	bool bad = false;

	if( i < numVertices ) {
		uint32_t slots[4];
		float blend[4];
		loadInfluence( influences, i, slots, blend );
		const float4 moved = ptm::posePosition( entries, runFirst[i], runFirst[i + 1], weights, bones, slots, blend, rest[i] );
		bad = !ptx::finitePosition( moved );
		staged[i] = moved;
	}

	raiseOncePerWave( bad, flag );
}

__global__ __launch_bounds__( 256 ) void poseNormals( const float4* __restrict__ rest, const uint32_t* __restrict__ runFirst,
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
	normals[i] = ptm::poseNormal( entries, runFirst[i], runFirst[i + 1], weights, bones, slots, blend, rest[i] );
}

}   // namespace ptr
