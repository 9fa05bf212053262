// pt_patch_refit_host.hpp — what pbr_update_geometry adds to the refit (pt_refit_host.hpp) for Phong tessellation: a face's
// THICK box, one source for both sides — the kernels of pt_patch_refit.hpp call it on the device, pbr_hip.hip's checks and
// tests/patch_refit_driver.cpp (a plain C++17 compiler, -ffp-contract=off like the library) on the host — and the thick refit
// of a whole tree in plain C++.  tests/patch_refit_ref.py restates both in numpy.
//
// The face box, operation by operation in binary32, none fused (include/pbr_hip.h, pbr_update_geometry, has it in full); it
// is host/bvh_builder.cpp's triBox with the refit's fold:
//   lo = hi = corner a; fold b, then c: lo = ( v < lo ) ? v : lo, hi = ( v > hi ) ? v : hi
//   if alpha > 0 and the three normals are not equal — t = ( n1 - n2 ) + ( n2 - n3 ), any fabsf( t.k ) > 0.000001f —
//   fold the raised corners p_k + thickness * ng, k = 1, 2, 3, then the nine edge points phongPoint( u, v ) of foldFace's table.
// A NaN point (a face without area has ng = NaN) fails both compares and never enters the fold; the corners are finite, so
// no box word is NaN.
#pragma once

#include <cmath>
#include <cstdint>

#include "pt_refit_host.hpp"

#if defined( __HIPCC__ )
#define PATCH_FN __host__ __device__ inline
#else
#define PATCH_FN inline
#endif

namespace ptp {

// glm's evaluation order, as host/bvh_builder.cpp has it: dot = ( x*x' + y*y' ) + z*z', normalize = v * ( 1 / sqrt( dot ) )
struct V3 {
	float x, y, z;
};

PATCH_FN V3 operator+( V3 a, V3 b ) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
PATCH_FN V3 operator-( V3 a, V3 b ) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
PATCH_FN V3 operator*( V3 a, float s ) { return { a.x * s, a.y * s, a.z * s }; }
PATCH_FN V3 operator*( float s, V3 a ) { return { s * a.x, s * a.y, s * a.z }; }
PATCH_FN float dot3( V3 a, V3 b ) { return ( a.x * b.x + a.y * b.y ) + a.z * b.z; }
PATCH_FN V3 cross3( V3 a, V3 b ) { return { a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y }; }
PATCH_FN V3 normalize3( V3 a ) { return a * ( 1.0f / sqrtf( dot3( a, a ) ) ); }
PATCH_FN V3 onPlane( V3 q, V3 p, V3 n ) { return q - dot3( q - p, n ) * n; }

PATCH_FN V3 phongPoint( const V3 p[3], const V3 n[3], float alpha, float u, float v ) {
	const float w = 1.0f - u - v;
	const V3 bary = ( p[0] * u + p[1] * v ) + p[2] * w;
	const V3 tess = ( u * onPlane( bary, p[0], n[0] ) + v * onPlane( bary, p[1], n[1] ) ) + w * onPlane( bary, p[2], n[2] );
	return ( 1.0f - alpha ) * bary + alpha * tess;
}

struct FaceBox {
	float lo[3], hi[3];
};

PATCH_FN void foldPoint( FaceBox& b, V3 v ) {
	b.lo[0] = ( v.x < b.lo[0] ) ? v.x : b.lo[0];
	b.lo[1] = ( v.y < b.lo[1] ) ? v.y : b.lo[1];
	b.lo[2] = ( v.z < b.lo[2] ) ? v.z : b.lo[2];
	b.hi[0] = ( v.x > b.hi[0] ) ? v.x : b.hi[0];
	b.hi[1] = ( v.y > b.hi[1] ) ? v.y : b.hi[1];
	b.hi[2] = ( v.z > b.hi[2] ) ? v.z : b.hi[2];
}

// Folds a face's twelve-or-three points into a running box: the three corners, then — alpha > 0, unequal normals — the
// raised corners and the edge points.  `start`: the box begins at corner a (a leaf's first face), else a is folded in too.
PATCH_FN void foldFace( FaceBox& b, bool start, const V3 p[3], const V3 n[3], float alpha ) {
	if( start ) {
		b = FaceBox { { p[0].x, p[0].y, p[0].z }, { p[0].x, p[0].y, p[0].z } };
	}
	else {
		foldPoint( b, p[0] );
	}

	foldPoint( b, p[1] );
	foldPoint( b, p[2] );

	if( !( alpha > 0.0f ) ) {
		return;
	}

	const V3 test = ( n[0] - n[1] ) + ( n[1] - n[2] );

	if( fabsf( test.x ) <= 0.000001f && fabsf( test.y ) <= 0.000001f && fabsf( test.z ) <= 0.000001f ) {
		return;   // equal normals: the patch is the flat triangle
	}

	const V3 e12 = p[1] - p[0], e13 = p[2] - p[0], e23 = p[2] - p[1], e31 = p[0] - p[2];
	const V3 c12 = alpha * ( dot3( n[1], e12 ) * n[1] - dot3( n[0], e12 ) * n[0] );
	const V3 c23 = alpha * ( dot3( n[2], e23 ) * n[2] - dot3( n[1], e23 ) * n[1] );
	const V3 c31 = alpha * ( dot3( n[0], e31 ) * n[0] - dot3( n[2], e31 ) * n[2] );
	const V3 ng = normalize3( cross3( e12, e13 ) );

	const float kTmp = dot3( ng, c12 - c23 - c31 );
	const float k = 1.0f / ( 4.0f * dot3( ng, c23 ) * dot3( ng, c31 ) - kTmp * kTmp );
	float u = k * ( 2.0f * dot3( ng, c23 ) * dot3( ng, c31 + e31 ) + dot3( ng, c23 - e23 ) * dot3( ng, c12 - c23 - c31 ) );
	float v = k * ( 2.0f * dot3( ng, c31 ) * dot3( ng, c23 - e23 ) + dot3( ng, c31 + e31 ) * dot3( ng, c12 - c23 - c31 ) );
	u = ( u < 0.0f || u > 1.0f ) ? 0.0f : u;
	v = ( v < 0.0f || v > 1.0f ) ? 0.0f : v;

	const V3 apex = phongPoint( p, n, alpha, u, v );
	const float thickness = dot3( ng, apex - p[0] );

	for( int c = 0; c < 3; c++ ) {
		foldPoint( b, p[c] + thickness * ng );
	}

	// host/bvh_builder.cpp's table, in its order
	const float edgeUV[9][2] = {
		{ 0.0f, 0.5f }, { 0.5f, 0.0f }, { 0.5f, 0.5f }, { 0.25f, 0.75f }, { 0.75f, 0.25f },
		{ 0.25f, 0.0f }, { 0.75f, 0.0f }, { 0.0f, 0.25f }, { 0.0f, 0.75f }
	};

	for( int s = 0; s < 9; s++ ) {
		foldPoint( b, phongPoint( p, n, alpha, edgeUV[s][0], edgeUV[s][1] ) );
	}
}

// The box of one face alone.  Folding a second face's box into a first one's with the same compares gives, bit for bit, the
// running fold over the first face's points and then the second's: minimum and maximum are exact, and among equal values (-0
// and +0) both keep the earliest — so a leaf's box can be made from two stored face boxes.
PATCH_FN FaceBox faceBox( const V3 p[3], const V3 n[3], float alpha ) {
	FaceBox b;
	foldFace( b, true, p, n, alpha );
	return b;
}

}   // namespace ptp

// ---- host only from here ----

inline void patchCorners( const pbr_uint4& fv, const pbr_uint4& fn, const pbr_float4* vertices, const pbr_float4* normals, ptp::V3 p[3], ptp::V3 n[3] ) {
	const uint32_t vi[3] = { fv.x, fv.y, fv.z }, ni[3] = { fn.x, fn.y, fn.z };

	for( int k = 0; k < 3; k++ ) {
		p[k] = { vertices[vi[k]].x, vertices[vi[k]].y, vertices[vi[k]].z };
		n[k] = { normals[ni[k]].x, normals[ni[k]].y, normals[ni[k]].z };
	}
}

// The thick refit in plain C++: the boxes of `nodes` (the tree's, N entries) from the vertices and normals under alpha; the
// .w words stay.  A leaf is ONE running fold over its first face's points, then its second's; containers as refitBoxes.
inline void patchRefitBoxes( const SceneTree& tree, const RefitPlan& plan, const pbr_uint4* facesV, const pbr_uint4* facesN,
                             const pbr_float4* vertices, const pbr_float4* normals, float alpha, pbr_bvh_node* nodes ) {
	for( uint32_t i = tree.size(); i-- > 0; ) {   // children come behind their parent
		float lo[3], hi[3];

		if( tree.face0s[i] >= 0 ) {
			const int faces = ( tree.links[i] >= 0 ) ? 2 : 1;
			ptp::FaceBox b;

			for( int f = 0; f < faces; f++ ) {
				ptp::V3 p[3], n[3];
				patchCorners( facesV[tree.face0s[i] + f], facesN[tree.face0s[i] + f], vertices, normals, p, n );
				ptp::foldFace( b, f == 0, p, n, alpha );
			}

			std::copy( b.lo, b.lo + 3, lo );
			std::copy( b.hi, b.hi + 3, hi );
		}
		else {
			refitContainerBox( plan, nodes, i, lo, hi );
		}

		refitStoreBox( nodes, i, lo, hi );
	}
}
