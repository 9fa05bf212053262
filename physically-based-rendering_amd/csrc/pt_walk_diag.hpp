// pbr_diag_trace_walk (include/pbr_hip_diag.h): one chosen ray per thread through the walk the lock-step render kernels run.
//
// diagTrace (pt_aux.hpp) instantiates traverse< false, LIGHTS, /*USE_LDS*/ false, PHONG >: the C++ node phase on the stream in
// memory, closest hit only.  The renders walk through the staged prefix — in product builds the hand-scheduled node phases
// nodePhaseAsm< ANYHIT > / nodePhaseAsmCompact< ANYHIT > — and their shade step runs the any-hit walk, which no other entry
// reaches.  This kernel is what stands around traverse() in pathTracing, and nothing else: the block stages the hot prefix
// (stageHotNodes), thread i walks ray i, one launch.  Wave = i / 64, lane = i % 64: the caller decides which rays share a node
// phase, who parks in which visit and how many lanes enter (`keep` of traverse()).
//
// Like the focus chain it is compiled once per build flavour (pt_flavour.hpp; pt_instance.hip, group PTI_WALK): the walk
// order, the record layout and the arithmetic are those of the context's configuration.  The kernel has no __shared__ data of
// its own: the staged prefix lies at LDS address 0, which is what the node phases address (stageHotNodes raises guard[3]
// otherwise, and the entry fails).
#pragma once

#include "pt_kernel.hpp"

namespace ptk {

// rays: n x { origin.xyz, t0 }{ dir.xyz, - }.  t0 is what hit.t starts from: tLight of the any-hit walk, +inf (or a finite
// bound) of the closest-hit walk.  Outputs as diagTrace's; node visits are counted by the closest-hit walk only (traverse()).
template<bool ANYHIT, bool LIGHTS, bool USE_LDS, bool PHONG>
__global__ __launch_bounds__( PBR_BLOCK, 4 ) void diagTraceWalk( const DevParams P, const float4* rays, unsigned n, float* outT, int* outFace, float* outNormal, unsigned* outCounts ) {
	const float4* lds = gHotNodes;

	// every thread of the block: stageHotNodes holds a __syncthreads
	if( USE_LDS ) {
		stageHotNodes( P, gHotNodes );
	}

	const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;

	if( i >= n ) {
		return;
	}

	const float4 a = rays[(size_t) i * 2 + 0];
	const float4 b = rays[(size_t) i * 2 + 1];
	Ray ray;
	ray.origin = mk3( a.x, a.y, a.z );
	ray.dir = mk3( b.x, b.y, b.z );
	Hit hit;
	hit.t = a.w;
	// No face index reaches this value (face * 3 + 2 indexes the records in an int), so it says "nothing was recorded": the walk
	// only ever assigns hit.face — a face's index, or -( i + 1 ) for an orb light — and never reads it.  t cannot say it: after an
	// orb in front of a finite t0 has set t to inf, a face may be recorded at exactly t0.
	const int kNoFace = 0x7fffffff;
	hit.face = kNoFace;
	hit.normal = mk3( 0.0f, 0.0f, 0.0f );
	unsigned nodes = 0, tris = 0;
	traverse<ANYHIT, LIGHTS, USE_LDS, PHONG>( P, lds, ray, hit, nodes, tris );

	const bool recorded = ( hit.face >= 0 && hit.face != kNoFace );

	if( hit.face == kNoFace ) {
		hit.face = 0;         // as the reference's ray starts out
	}

	f3 normal = mk3( 0.0f, 0.0f, 0.0f );

	if( !ANYHIT && recorded ) {
		if( PHONG ) {
			normal = hit.normal;
		}
		else {
			int material;
			normal = faceNormal( P, hit.face, &material );
		}
	}

	outT[i] = hit.t;
	outFace[i] = hit.face;
	outNormal[(size_t) i * 3 + 0] = normal.x;
	outNormal[(size_t) i * 3 + 1] = normal.y;
	outNormal[(size_t) i * 3 + 2] = normal.z;
	outCounts[(size_t) i * 2 + 0] = nodes;
	outCounts[(size_t) i * 2 + 1] = tris;
}

}  // namespace ptk
