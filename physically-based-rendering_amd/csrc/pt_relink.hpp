// pt_relink.hpp — the kernels behind pbr_update_vertices while pbr_refit_ordered_walk is on and a ray-ordered traversal is
// configured (host side: pbr_hip.hip; the tables and the per-item bodies: pt_relink_host.hpp, which states the algorithm).
// They run behind refitTop on the same stream, so the kernel boundary makes the refitted boxes visible.
//
//   relinkSortKernel     one thread per container: its axis, its sorted child lists
//   relinkLevelsKernel   one thread per (container, order) of a level: the children's next and pos.  A wide level is a launch of
//                        its own; consecutive narrow levels share a launch of ONE workgroup, a workgroup barrier between two
//                        levels (as refitTop does bottom-up).  A level reads what the level above wrote — across a kernel
//                        boundary or that barrier, never from another workgroup of the same launch: per-XCD L2s are not coherent
//                        without agent-scope fences
//   relinkRecordsKernel  one thread per (node, stream): the record; thread 0 of stream 0 writes the header
//
// No atomics, no inline assembly; the threads of a launch write disjoint words.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_relink_host.hpp"

#define RELINK_THREADS 256          // = kRelinkWideThreads
#define RELINK_NARROW_THREADS 1024  // = kRelinkNarrowThreads

namespace ptl {

__global__ __launch_bounds__( RELINK_THREADS ) void relinkSortKernel( const RelinkView v, const unsigned* __restrict__ containers, unsigned numContainers ) {
	const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;

	if( t < numContainers ) {
		relinkSort( v, containers[t] );
	}
}

// levelFirst: of the whole tree.  numLevels > 1 only with gridDim.x == 1.
__global__ __launch_bounds__( RELINK_NARROW_THREADS ) void relinkLevelsKernel( const RelinkView v, const unsigned* __restrict__ levelNodes,
                                                                              const unsigned* __restrict__ levelFirst, unsigned firstLevel, unsigned numLevels ) {
	for( unsigned level = firstLevel; level < firstLevel + numLevels; level++ ) {
		const unsigned first = levelFirst[level], count = levelFirst[level + 1] - first;
		const unsigned total = count * v.K;

		// order-major: neighbouring threads take neighbouring containers of one order
		for( unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x ) {
			relinkLevel( v, levelNodes[first + t % count], t / count );
		}

		if( numLevels > 1 ) {
			__syncthreads();   // workgroup scope: the next level reads this one's next and pos
		}
	}
}

__global__ __launch_bounds__( RELINK_THREADS ) void relinkRecordsKernel( const RelinkView v ) {
	const unsigned n = 1u + blockIdx.x * blockDim.x + threadIdx.x;
	const unsigned k = blockIdx.y;

	if( n >= v.N ) {
		return;
	}

	if( v.compact ) {
		relinkRecordCompact( v, n );
	}
	else {
		relinkRecord32( v, n, k );
	}

	if( n == 1u && k == 0u ) {
		relinkHeader( v );
	}
}

}   // namespace ptl
