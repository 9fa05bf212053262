// pt_skin.hpp — the kernels pbr_update_skin puts in front of the refit's (pt_refit.hpp, pt_patch_refit.hpp; host side:
// pbr_hip.hip).  Both stream: one thread per vertex / per normal, one 16-byte load of the rest quad, two 16-byte loads of the
// element's influence record (four bones, four weights: pts::Influence), three 16-byte loads of a 48-byte bone record per slot
// whose weight is not 0, one 16-byte store — 64 bytes of unavoidable traffic per element, the bone records on top.
//
//   skinVertices  V' = B * rest into a STAGING buffer, B the blend of the element's bones (pt_skin_host.hpp, pts::skinPosition:
//                 the same source the host unit is built from).  A position with a word that is not finite raises *flag —
//                 once per wave: a ballot, then the first lane that saw one stores a 1 (plain store; every writer stores the
//                 same word), exactly as transformVertices does.  The host reads the flag before the staging buffer becomes
//                 the context's vertices.
//   skinNormals   N' = normalize( cof( B ) * rest ) straight into the patch refit's normal table; it cannot fail.  The nine
//                 cofactor words are computed per element here: B differs from element to element.
//
// The bone records are NOT staged in LDS, on pt_transform.hpp's argument: a record is 48 bytes, neighbours in the array mostly
// share their bones, so the 64 lanes of a wave fetch a handful of records from a few cache lines and the CU's vector L1 holds
// several hundred of them.  Staging would read the whole table once per workgroup of 256 elements — more bytes than the
// elements themselves from about 340 bones on — and add a barrier to a kernel that has none.  Unmeasured against the
// alternative.  No workgroup talks to another, there is no atomic and no LDS here.
//
// Bounds: the host has checked every bone index against the bone count before the influence records were uploaded
// (checkSkin: zero-weight slots too), `influences` holds two quads per element and `bones` three per bone.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_skin_host.hpp"

namespace ptr {

__device__ inline void loadInfluence( const uint4* __restrict__ influences, int i, uint32_t bones[4], float weights[4] ) {
	const uint4 b = influences[(size_t) i * 2], w = influences[(size_t) i * 2 + 1];
	bones[0] = b.x;
	bones[1] = b.y;
	bones[2] = b.z;
	bones[3] = b.w;
	weights[0] = __uint_as_float( w.x );
	weights[1] = __uint_as_float( w.y );
	weights[2] = __uint_as_float( w.z );
	weights[3] = __uint_as_float( w.w );
}

__global__ __launch_bounds__( 256 ) void skinVertices( const float4* __restrict__ rest, const uint4* __restrict__ influences,
                                                       const float4* __restrict__ bones, float4* __restrict__ staged,
                                                       unsigned* __restrict__ flag, int numVertices ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );
	bool bad = false;

	if( i < numVertices ) {
		uint32_t slots[4];
		float weights[4];
		const float4 p = rest[i];
		loadInfluence( influences, i, slots, weights );
		const float4 moved = pts::skinPosition( bones, slots, weights, p );
		bad = !ptx::finitePosition( moved );
		staged[i] = moved;
	}

	const unsigned long long raised = __ballot( bad );

	if( bad && ( raised & ( ( 1ull << ( threadIdx.x & 63u ) ) - 1ull ) ) == 0ull ) {
		*flag = 1u;
	}
}

__global__ __launch_bounds__( 256 ) void skinNormals( const float4* __restrict__ rest, const uint4* __restrict__ influences,
                                                      const float4* __restrict__ bones, float4* __restrict__ normals, int numNormals ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( i >= numNormals ) {
		return;
	}

	uint32_t slots[4];
	float weights[4];
	const float4 n = rest[i];
	loadInfluence( influences, i, slots, weights );
	normals[i] = pts::skinNormal( bones, slots, weights, n );
}

}   // namespace ptr
