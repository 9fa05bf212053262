// pt_transform.hpp — the kernels pbr_update_transforms puts in front of the refit's (pt_refit.hpp, pt_patch_refit.hpp; host
// side: pbr_hip.hip).  Both stream: one thread per vertex / per normal, one 16-byte load of the rest word quad, one 4-byte load
// of its part index, three 16-byte loads of the part's record through that index, one 16-byte store — 36 bytes of unavoidable
// traffic per element, the record loads on top.
//
//   transformVertices  V' = M[part] * rest into a STAGING buffer (pt_transform_host.hpp, ptx::transformPosition: the same source
//                      the host unit is built from).  A position with a word that is not finite raises *flag — once per wave:
//                      a ballot, then the first lane that saw one stores a 1 (plain store; every writer stores the same word).
//                      The host reads the flag before the staging buffer becomes the context's vertices.
//   transformNormals   N' = normalize( cof( M[part] ) * rest ) straight into the patch refit's normal table; it cannot fail.
//
// The records are NOT staged in LDS.  A record is 96 bytes and a kernel reads 48 of them; the vertices of a part are mostly
// neighbours in the array, so the 64 lanes of a wave fetch one or two records from a few cache lines and the CU's vector L1
// holds hundreds of records.  Staging would read the whole table once per workgroup of 256 elements — more bytes than the
// elements themselves from a few dozen parts on — and add a barrier to a kernel that has none.  Unmeasured against the
// alternative.  No workgroup talks to another, there is no atomic and no LDS here.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_transform_host.hpp"

namespace ptr {

__global__ __launch_bounds__( 256 ) void transformVertices( const float4* __restrict__ rest, const unsigned* __restrict__ part,
                                                            const float4* __restrict__ records, float4* __restrict__ staged,
                                                            unsigned* __restrict__ flag, int numVertices ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );
	bool bad = false;

	if( i < numVertices ) {
		const float4 p = rest[i];
		const float4* record = records + (size_t) part[i] * 6;
		const float4 r0 = record[0], r1 = record[1], r2 = record[2];
		const float m[12] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w };
		const float4 moved = ptx::transformPosition( m, p );
		bad = !ptx::finitePosition( moved );
		staged[i] = moved;
	}

	const unsigned long long raised = __ballot( bad );

	if( bad && ( raised & ( ( 1ull << ( threadIdx.x & 63u ) ) - 1ull ) ) == 0ull ) {
		*flag = 1u;
	}
}

__global__ __launch_bounds__( 256 ) void transformNormals( const float4* __restrict__ rest, const unsigned* __restrict__ part,
                                                           const float4* __restrict__ records, float4* __restrict__ normals, int numNormals ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( i >= numNormals ) {
		return;
	}

	const float4 n = rest[i];
	const float4* record = records + (size_t) part[i] * 6;
	const float4 r3 = record[3], r4 = record[4], r5 = record[5];
	const float c[9] = { r3.x, r3.y, r3.z, r3.w, r4.x, r4.y, r4.z, r4.w, r5.x };
	normals[i] = ptx::transformNormal( c, __float_as_uint( r5.y ) != 0u, n );
}

}   // namespace ptr
