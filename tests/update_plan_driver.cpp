// Exposes the host-only unit of the six update calls (physically-based-rendering_amd/csrc/pt_update_host.hpp — the refusals
// pbr_hip.hip's updateScene asks for before it touches the device, and the plan of what an admitted call launches) to
// tests/test_update_plan_cpu.py through ctypes: plain C++17, built with g++ -shared like its sibling tests/morph_driver.cpp.
//   up_call          the kind's name as the messages print it
//   up_admit_kind    stage 1: the kind's own state refusal
//   up_admit_shared  stage 3: the refusals every update shares (the kind's argument check runs between the two, in its own unit)
//   up_plan          { ordered, gathers, relinks, keepsHistory, normal kernel } and alpha of an admitted call
//   up_last          what the context reports of a most recent update of this kind: { a pbr_update_geometry, the morph's code }
// With -DUPDATE_PLAN_DRIVER_MAIN it is a program of its own: every kind through both stages and the plan, with a reason longer
// than the message buffer, for a run under the host sanitizers (the messages are formatted into a fixed buffer).
#include <cstdio>
#include <cstring>
#include <string>

#include "pt_update_host.hpp"

extern "C" {

// UpdateFacts as ctypes passes it: every bool an int
struct up_facts {
	int32_t hasScene, nested, configured;
	uint32_t traversal;
	float phongTessellation;
	int32_t refitOrdered, hasPatches, walkBuilt;
	uint32_t numParts, numBones, numMorphTargets;
	uint64_t skinGeneration, morphGeneration;
	int32_t partNormals, skinNormals, morphNormals, tracking, history, moved;
};

}  // extern "C"

namespace {

UpdateFacts factsOf( const up_facts* in, const char* reason ) {
	UpdateFacts f;
	f.hasScene = in->hasScene != 0;
	f.nested = in->nested != 0;
	f.why = reason;
	f.configured = in->configured != 0;
	f.traversal = in->traversal;
	f.phongTessellation = in->phongTessellation;
	f.refitOrdered = in->refitOrdered != 0;
	f.hasPatches = in->hasPatches != 0;
	f.walkBuilt = in->walkBuilt != 0;
	f.numParts = in->numParts;
	f.numBones = in->numBones;
	f.numMorphTargets = in->numMorphTargets;
	f.skinGeneration = in->skinGeneration;
	f.morphGeneration = in->morphGeneration;
	f.partNormals = in->partNormals != 0;
	f.skinNormals = in->skinNormals != 0;
	f.morphNormals = in->morphNormals != 0;
	f.tracking = in->tracking != 0;
	f.history = in->history != 0;
	f.moved = in->moved != 0;
	return f;
}

}  // namespace

extern "C" {

const char* up_call( uint32_t kind ) {
	return updateCall( (UpdateKind) kind );
}

int up_admit_kind( uint32_t kind, const up_facts* facts, char* why, size_t capacity ) {
	std::string error;
	const int status = admitKind( (UpdateKind) kind, factsOf( facts, "" ), &error );
	std::snprintf( why, capacity, "%s", error.c_str() );
	return status;
}

int up_admit_shared( uint32_t kind, int brings_normals, const up_facts* facts, const char* reason, char* why, size_t capacity ) {
	std::string error;
	const int status = admitShared( (UpdateKind) kind, brings_normals != 0, factsOf( facts, reason ), &error );
	std::snprintf( why, capacity, "%s", error.c_str() );
	return status;
}

void up_plan( uint32_t kind, const up_facts* facts, int32_t out[5], float* alpha ) {
	const UpdatePlan plan = planUpdate( (UpdateKind) kind, factsOf( facts, "" ) );
	out[0] = plan.ordered ? 1 : 0;
	out[1] = plan.gathers ? 1 : 0;
	out[2] = plan.relinks ? 1 : 0;
	out[3] = plan.keepsHistory ? 1 : 0;
	out[4] = (int32_t) plan.normals;
	*alpha = plan.alpha;
}

void up_last( uint32_t kind, uint32_t out[2] ) {
	out[0] = updateWasGeometry( (UpdateKind) kind ) ? 1u : 0u;
	out[1] = updateMorphCode( (UpdateKind) kind );
}

}  // extern "C"

#ifdef UPDATE_PLAN_DRIVER_MAIN
// Every kind: refused by its own state on an empty context, admitted on a full one, refused by a tree that is not nested with a
// reason of 700 characters — more than the message buffer holds —, and planned.
int main() {
	const std::string reason( 700, 'x' );
	up_facts empty;
	std::memset( &empty, 0, sizeof( empty ) );
	up_facts full = empty;
	full.hasScene = full.nested = full.configured = full.refitOrdered = full.hasPatches = full.walkBuilt = 1;
	full.traversal = 2;
	full.phongTessellation = 0.5f;
	full.numParts = full.numBones = full.numMorphTargets = 3;
	full.skinGeneration = full.morphGeneration = 7;
	full.partNormals = full.skinNormals = full.morphNormals = full.tracking = full.history = 1;
	up_facts loose = full;
	loose.nested = 0;
	const int32_t wantNormals[7] = { 0, 0, 0, 1, 2, 3, 4 };
	char why[1024];

	for( uint32_t kind = 1; kind <= 6; kind++ ) {
		if( up_admit_kind( kind, &empty, why, sizeof( why ) ) != PBR_ESTATE || std::strstr( why, up_call( kind ) ) == nullptr ) {
			std::printf( "kind %u on an empty context: %s\n", kind, why );
			return 1;
		}
		if( up_admit_kind( kind, &full, why, sizeof( why ) ) != PBR_OK || why[0] != 0 ) {
			return 2;
		}
		if( up_admit_shared( kind, 0, &loose, reason.c_str(), why, sizeof( why ) ) != PBR_ESTATE || std::strlen( why ) != 511 ) {
			std::printf( "kind %u, not nested: %zu characters\n", kind, std::strlen( why ) );
			return 3;
		}
		// kind 1, pbr_update_vertices, is refused under the Phong tessellation the full context has configured
		if( up_admit_shared( kind, 0, &full, "", why, sizeof( why ) ) != ( kind == 1 ? PBR_ESTATE : PBR_OK ) ) {
			return 4;
		}

		int32_t plan[5];
		float alpha = -1.0f;
		up_plan( kind, &full, plan, &alpha );

		if( plan[0] != 1 || plan[1] != ( kind == 1 ? 0 : 1 ) || plan[2] != 1 || plan[3] != 1 || plan[4] != wantNormals[kind] || alpha != ( kind == 1 ? 0.0f : 0.5f ) ) {
			std::printf( "kind %u: plan %d %d %d %d %d, alpha %g\n", kind, plan[0], plan[1], plan[2], plan[3], plan[4], (double) alpha );
			return 5;
		}

		uint32_t last[2];
		up_last( kind, last );

		if( last[0] != ( kind == 1 ? 0u : 1u ) || last[1] != ( kind == 5 ? 1u : kind == 6 ? 2u : 0u ) ) {
			return 6;
		}
	}

	std::printf( "update plan driver ok\n" );
	return 0;
}
#endif
