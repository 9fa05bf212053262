// pt_refit.hpp — the kernels of pbr_update_vertices (host side: pbr_hip.hip; the tables they read: pt_refit_host.hpp).
//
//   refitFaces     one thread per face: the face record {a, b - a, c - a, material} from the new vertices (packScene's lines;
//                  a subtraction alone cannot contract, and the library is built with -ffp-contract=off anyway)
//   refitSubtrees  one workgroup per group of maximal subtrees of at most REFIT_SUBTREE nodes, one thread slot per node: leaf
//                  boxes from the corners, then the containers height by height over LDS behind a workgroup barrier; every
//                  box is stored once, box words only, into the node's record of the reference-order stream.  Its PHONG build
//                  (pbr_update_geometry under Phong tessellation) makes a leaf's box from the thick boxes of its faces, which
//                  refitPatches (pt_patch_refit.hpp) stored one launch earlier; everything behind the leaf step is the same
//   refitTop       the nodes above the cut, one workgroup: level by level (lowest first) from the children's records, a
//                  workgroup barrier between two levels — launched behind refitSubtrees, so the kernel boundary makes the
//                  subtree roots' records visible
//
// No workgroup talks to another one: per-XCD L2s are not coherent without agent-scope fences, and a climb in which the last
// child to arrive carries on needs one per node.  A container's box is a fold over all its children in depth-first child
// order (pt_refit_host.hpp states it operation by operation), never an accumulation by arrival, so it does not depend on the
// schedule.
#pragma once

#include <hip/hip_runtime.h>

#define REFIT_SUBTREE 256   // = kRefitSubtree (pt_refit_host.hpp): thread slots, and nodes, per workgroup
#define REFIT_TOP_THREADS 1024

namespace ptr {

struct Box {
	float lo[3], hi[3];
};

__device__ inline void foldPoint( Box& b, const float4 v ) {
	b.lo[0] = ( v.x < b.lo[0] ) ? v.x : b.lo[0];
	b.lo[1] = ( v.y < b.lo[1] ) ? v.y : b.lo[1];
	b.lo[2] = ( v.z < b.lo[2] ) ? v.z : b.lo[2];
	b.hi[0] = ( v.x > b.hi[0] ) ? v.x : b.hi[0];
	b.hi[1] = ( v.y > b.hi[1] ) ? v.y : b.hi[1];
	b.hi[2] = ( v.z > b.hi[2] ) ? v.z : b.hi[2];
}

__device__ inline void foldBox( Box& b, const Box& c ) {
#pragma unroll
	for( int k = 0; k < 3; k++ ) {
		b.lo[k] = ( c.lo[k] < b.lo[k] ) ? c.lo[k] : b.lo[k];
		b.hi[k] = ( c.hi[k] > b.hi[k] ) ? c.hi[k] : b.hi[k];
	}
}

// a leaf's box: corner a of its first face, then b, c, then the second face's corners
__device__ inline Box leafBox( unsigned word, const uint4* facesV, const float4* vertices ) {
	const unsigned face = word & 0x3FFFFFFFu;
	const uint4 f0 = facesV[face];
	const float4 a = vertices[f0.x];
	Box b = { { a.x, a.y, a.z }, { a.x, a.y, a.z } };
	foldPoint( b, vertices[f0.y] );
	foldPoint( b, vertices[f0.z] );

	if( word & 0x40000000u ) {
		const uint4 f1 = facesV[face + 1];
		foldPoint( b, vertices[f1.x] );
		foldPoint( b, vertices[f1.y] );
		foldPoint( b, vertices[f1.z] );
	}

	return b;
}

// ... and under Phong tessellation: the first face's stored thick box, then the second face's folded in — bit for bit the
// running fold over the first face's points and then the second's (pt_patch_refit_host.hpp, faceBox)
__device__ inline Box loadFaceBox( const float2* faceBoxes, unsigned face ) {
	const float2 q0 = faceBoxes[(size_t) face * 3 + 0], q1 = faceBoxes[(size_t) face * 3 + 1], q2 = faceBoxes[(size_t) face * 3 + 2];
	return Box { { q0.x, q0.y, q1.x }, { q1.y, q2.x, q2.y } };
}

__device__ inline Box leafBoxThick( unsigned word, const float2* faceBoxes ) {
	const unsigned face = word & 0x3FFFFFFFu;
	Box b = loadFaceBox( faceBoxes, face );

	if( word & 0x40000000u ) {
		foldBox( b, loadFaceBox( faceBoxes, face + 1 ) );
	}

	return b;
}

// The record of the reference-order stream (pt_scene_pack.hpp, encodeRecords32): {lo.x, lo.y, hi.x, hi.y} {lo.z, hi.z, word,
// word}.  Node 0 has no record (record < 0): its box goes to rootBox, in the wire format's order.
__device__ inline void storeBox( float4* nodes, float4* rootBox, int record, const Box& b ) {
	if( record < 0 ) {
		rootBox[0] = make_float4( b.lo[0], b.lo[1], b.lo[2], -1.0f );
		rootBox[1] = make_float4( b.hi[0], b.hi[1], b.hi[2], -1.0f );
		return;
	}

	nodes[(size_t) record * 2] = make_float4( b.lo[0], b.lo[1], b.hi[0], b.hi[1] );
	*reinterpret_cast<float2*>( nodes + (size_t) record * 2 + 1 ) = make_float2( b.lo[2], b.hi[2] );
}

__device__ inline Box loadBox( const float4* nodes, int record ) {
	const float4 r0 = nodes[(size_t) record * 2];
	const float2 r1 = *reinterpret_cast<const float2*>( nodes + (size_t) record * 2 + 1 );
	return Box { { r0.x, r0.y, r1.x }, { r0.z, r0.w, r1.y } };
}

__global__ __launch_bounds__( 256 ) void refitFaces( const uint4* __restrict__ facesV, const float4* __restrict__ vertices, float4* __restrict__ tris, int numFaces ) {
	const int f = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( f >= numFaces ) {
		return;
	}

	const uint4 fv = facesV[f];
	const float4 a = vertices[fv.x];
	const float4 b = vertices[fv.y];
	const float4 c = vertices[fv.z];
	const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
	const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
	tris[(size_t) f * 3 + 0] = make_float4( a.x, a.y, a.z, e1x );
	tris[(size_t) f * 3 + 1] = make_float4( e1y, e1z, e2x, e2y );
	tris[(size_t) f * 3 + 2] = make_float4( e2z, __int_as_float( (int) fv.w ), 0.0f, 0.0f );
}

template<bool PHONG>
__global__ __launch_bounds__( REFIT_SUBTREE ) void refitSubtrees( const unsigned* __restrict__ slots, const unsigned* __restrict__ info,
                                                                  const unsigned short* __restrict__ heights, const int* __restrict__ recordOf,
                                                                  const uint4* __restrict__ facesV, const float4* __restrict__ vertices,
                                                                  const float2* __restrict__ faceBoxes, float4* nodes, float4* rootBox ) {
	__shared__ float sBox[6][REFIT_SUBTREE];
	__shared__ unsigned sInfo[REFIT_SUBTREE];

	const unsigned slot = threadIdx.x;
	const unsigned node = slots[(size_t) blockIdx.x * REFIT_SUBTREE + slot];
	const bool valid = ( node != 0xFFFFFFFFu );
	const unsigned word = valid ? info[node] : 0x80000000u;
	const unsigned height = valid ? heights[node] : 0u;
	sInfo[slot] = word;
	Box b = {};

	if( valid && height == 0u ) {
		b = PHONG ? leafBoxThick( word, faceBoxes ) : leafBox( word, facesV, vertices );

		for( int k = 0; k < 3; k++ ) {
			sBox[k][slot] = b.lo[k];
			sBox[3 + k][slot] = b.hi[k];
		}
	}

	// level h reads what the levels below it wrote before an earlier barrier; the loop count is the same for all threads
	for( unsigned h = 1; __syncthreads_or( valid && height >= h ); h++ ) {
		if( valid && height == h ) {
			// a subtree is a contiguous index range, so child c of `node` sits in slot + ( c - node )
			unsigned c = node + 1u;

			for( bool first = true; c < word; first = false ) {
				const unsigned at = slot + ( c - node );
				const Box child = { { sBox[0][at], sBox[1][at], sBox[2][at] }, { sBox[3][at], sBox[4][at], sBox[5][at] } };

				if( first ) {
					b = child;
				}
				else {
					foldBox( b, child );
				}

				const unsigned cw = sInfo[at];
				c = ( cw & 0x80000000u ) ? c + 1u : cw;
			}

			for( int k = 0; k < 3; k++ ) {
				sBox[k][slot] = b.lo[k];
				sBox[3 + k][slot] = b.hi[k];
			}
		}
	}

	if( valid ) {
		storeBox( nodes, rootBox, recordOf[node], b );
	}
}

__global__ __launch_bounds__( REFIT_TOP_THREADS ) void refitTop( const unsigned* __restrict__ topNodes, const unsigned* __restrict__ levelFirst, int numLevels,
                                                                 const unsigned* __restrict__ info, const int* __restrict__ recordOf,
                                                                 float4* nodes, float4* rootBox ) {
	for( int level = 0; level < numLevels; level++ ) {
		const unsigned first = levelFirst[level], last = levelFirst[level + 1];

		for( unsigned k = first + threadIdx.x; k < last; k += blockDim.x ) {
			const unsigned node = topNodes[k];
			const unsigned end = info[node];   // above the cut there are containers only
			unsigned c = node + 1u;
			Box b = loadBox( nodes, recordOf[c] );
			unsigned cw = info[c];
			c = ( cw & 0x80000000u ) ? c + 1u : cw;

			while( c < end ) {
				foldBox( b, loadBox( nodes, recordOf[c] ) );
				cw = info[c];
				c = ( cw & 0x80000000u ) ? c + 1u : cw;
			}

			storeBox( nodes, rootBox, recordOf[node], b );
		}

		__syncthreads();   // workgroup scope: the next level reads this one's records
	}
}

}   // namespace ptr
