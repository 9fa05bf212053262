// Exposes the host-only unit of pbr_update_vertices (physically-based-rendering_amd/csrc/pt_refit_host.hpp) to
// tests/test_refit_cpu.py through ctypes: built with g++ -shared -ffp-contract=off, fed the pbr_scene_desc the library takes.
//   rf_plan      checks a scene, packs its reference-order stream and plans the refit for subtrees of at most `cap` nodes;
//                null + status + message when the scene itself is refused (a tree that is merely not nested gives a plan)
//   rf_info      nested, nodes, workgroups, subtrees, nodes above the cut, their levels
//   rf_why       the reason of a "not nested" verdict
//   rf_array     0 parent, 1 end, 2 height, 3 subtreeRoots, 4 groupFirst, 5 slots, 6 topNodes, 7 topLevelFirst, 8 info
//   rf_record_of node -> record of the reference-order stream
//   rf_refit     the plain C++ refit: nodes_out = the scene's nodes with the boxes of `vertices`
//   rf_check_vertices  what pbr_update_vertices answers to these vertices before it touches the context
#include <cstdio>
#include <string>

#include "pt_refit_host.hpp"

namespace {

struct Planned {
	SceneTree tree;
	RefitPlan plan;
};

}  // namespace

extern "C" {

void* rf_plan( const pbr_scene_desc* s, uint32_t cap, int* status, char* why, size_t capacity ) {
	Planned* p = new Planned();
	PackedWalk walk;
	std::string error;
	*status = checkScene( s, &p->tree, &error );

	if( *status == PBR_OK ) {
		*status = packWalk( p->tree, 0, &walk, &error );
	}

	std::snprintf( why, capacity, "%s", error.c_str() );

	if( *status != PBR_OK ) {
		delete p;
		return nullptr;
	}

	planRefit( p->tree, walk.recordOf, cap, &p->plan );
	return p;
}

void rf_info( void* h, uint32_t* out ) {
	const Planned* p = (const Planned*) h;
	out[0] = p->plan.nested ? 1u : 0u;
	out[1] = p->tree.size();
	out[2] = p->plan.numGroups();
	out[3] = (uint32_t) p->plan.subtreeRoots.size();
	out[4] = (uint32_t) p->plan.topNodes.size();
	out[5] = p->plan.numLevels();
}

void rf_why( void* h, char* why, size_t capacity ) {
	std::snprintf( why, capacity, "%s", ( (const Planned*) h )->plan.why.c_str() );
}

size_t rf_array( void* h, int which, const uint32_t** data ) {
	const RefitPlan& plan = ( (const Planned*) h )->plan;
	const std::vector<uint32_t>* const arrays[9] = { &plan.parent, &plan.end, &plan.height, &plan.subtreeRoots, &plan.groupFirst,
	                                                 &plan.slots, &plan.topNodes, &plan.topLevelFirst, &plan.info };
	*data = arrays[which]->data();
	return arrays[which]->size();
}

size_t rf_record_of( void* h, const int** data ) {
	const RefitPlan& plan = ( (const Planned*) h )->plan;
	*data = plan.recordOf.data();
	return plan.recordOf.size();
}

int rf_refit( void* h, const pbr_uint4* facesV, const pbr_float4* vertices, pbr_bvh_node* nodes_out ) {
	const Planned* p = (const Planned*) h;

	if( !p->plan.nested ) {
		return PBR_ESTATE;
	}

	std::copy( p->tree.bvh.begin(), p->tree.bvh.end(), nodes_out );
	refitBoxes( p->tree, p->plan, facesV, vertices, nodes_out );
	return PBR_OK;
}

int rf_check_vertices( const pbr_float4* vertices, uint32_t num_vertices, uint32_t uploaded, char* why, size_t capacity ) {
	std::string error;
	const int status = checkRefitVertices( vertices, num_vertices, uploaded, &error );
	std::snprintf( why, capacity, "%s", error.c_str() );
	return status;
}

void rf_free( void* h ) {
	delete (Planned*) h;
}

}  // extern "C"
