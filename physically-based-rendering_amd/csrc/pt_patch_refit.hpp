// pt_patch_refit.hpp — the kernel pbr_update_geometry adds in front of the refit's (pt_refit.hpp; host side: pbr_hip.hip).
//
//   refitPatches<BOXES>  one thread per face: gathers the three corners and the three vertex normals through facesV / facesN
//                        into the Phong patch record of dTriPN — six quads, corners then normals, .w = 0 (packScene's layout) —
//                        and, BOXES, folds the face's thick box (pt_patch_refit_host.hpp, ptp::faceBox: the same source the host
//                        unit is built from) out of the registers it has just gathered and stores it, 24 bytes, into a per-face
//                        scratch table
//
// refitSubtrees<true> (pt_refit.hpp) then makes a leaf's box from its one or two stored face boxes.  The kernel boundary is
// the only ordering between the two; no workgroup talks to another, there is no atomic and no LDS here.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_patch_refit_host.hpp"

namespace ptr {

template<bool BOXES>
__global__ __launch_bounds__( 256 ) void refitPatches( const uint4* __restrict__ facesV, const uint4* __restrict__ facesN,
                                                       const float4* __restrict__ vertices, const float4* __restrict__ normals,
                                                       float4* __restrict__ triPN, float2* __restrict__ faceBoxes, float alpha, int numFaces ) {
	const int f = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( f >= numFaces ) {
		return;
	}

	const uint4 fv = facesV[f];
	const uint4 fn = facesN[f];
	const unsigned vi[3] = { fv.x, fv.y, fv.z }, ni[3] = { fn.x, fn.y, fn.z };
	ptp::V3 p[3], n[3];

#pragma unroll
	for( int k = 0; k < 3; k++ ) {
		const float4 v = vertices[vi[k]];
		const float4 m = normals[ni[k]];
		p[k] = { v.x, v.y, v.z };
		n[k] = { m.x, m.y, m.z };
		triPN[(size_t) f * 6 + k] = make_float4( v.x, v.y, v.z, 0.0f );
		triPN[(size_t) f * 6 + 3 + k] = make_float4( m.x, m.y, m.z, 0.0f );
	}

	if( BOXES ) {
		const ptp::FaceBox b = ptp::faceBox( p, n, alpha );
		faceBoxes[(size_t) f * 3 + 0] = make_float2( b.lo[0], b.lo[1] );
		faceBoxes[(size_t) f * 3 + 1] = make_float2( b.lo[2], b.hi[0] );
		faceBoxes[(size_t) f * 3 + 2] = make_float2( b.hi[1], b.hi[2] );
	}
}

}   // namespace ptr
