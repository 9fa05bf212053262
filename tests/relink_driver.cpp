// Exposes the host-only unit of the re-link (physically-based-rendering_amd/csrc/pt_relink_host.hpp) to
// tests/test_relink_cpu.py through ctypes: built with g++ -shared -ffp-contract=off, fed the pbr_scene_desc the library takes.
//   rl_run        checks scene S (the ranking is S's, shortened to `hot` nodes when hot >= 0), plans the refit, and builds the
//                 records of `layout` twice for the tree with the boxes of `boxes` (N nodes in the wire format; the .w words are
//                 S's): 0 packWalk on that tree, 1 relinkWalk; null + status + message when either refuses
//   rl_bytes      the storage of 0 / 1, header included
//   rl_info       hotSlots and first[8] of 0 / 1
//   rl_record_of  node -> record per stream of 0 / 1
//   rl_tables     of the re-link: levels, launches of the levels kernel, containers, device bytes of its tables, hot nodes per stream
#include <cstdio>
#include <string>

#include "pt_relink_host.hpp"

namespace {

struct Run {
	PackedWalk walk[2];
	RelinkTables tables;
};

}  // namespace

extern "C" {

void* rl_run( const pbr_scene_desc* s, const pbr_bvh_node* boxes, uint32_t layout, int hot, int* status, char* why, size_t capacity ) {
	Run* r = new Run();
	SceneTree tree;
	PackedWalk reference;
	RefitPlan plan;
	std::string error;
	*status = checkScene( s, &tree, &error );

	if( *status == PBR_OK && hot >= 0 && (size_t) hot < tree.ranked.size() ) {
		tree.ranked.resize( (size_t) hot );
	}
	if( *status == PBR_OK ) {
		*status = packWalk( tree, 0, &reference, &error );
	}
	if( *status == PBR_OK ) {
		planRefit( tree, reference.recordOf, kRefitSubtree, &plan );
		*status = relinkTables( tree, plan, layout, &r->tables, &error );
	}
	if( *status == PBR_OK ) {
		*status = relinkWalk( tree, plan, layout, boxes, &r->walk[1], &error );
	}
	if( *status == PBR_OK ) {
		for( uint32_t i = 0; i < tree.size(); i++ ) {
			const float w0 = tree.bvh[i].bbMin.w, w1 = tree.bvh[i].bbMax.w;
			tree.bvh[i] = boxes[i];
			tree.bvh[i].bbMin.w = w0;
			tree.bvh[i].bbMax.w = w1;
		}

		*status = packWalk( tree, layout, &r->walk[0], &error );
	}

	std::snprintf( why, capacity, "%s", error.c_str() );

	if( *status != PBR_OK ) {
		delete r;
		return nullptr;
	}

	return r;
}

size_t rl_bytes( void* h, int which, const void** data ) {
	const PackedWalk& walk = ( (const Run*) h )->walk[which];
	*data = walk.storage.data();
	return walk.storage.size() * sizeof( Quad );
}

void rl_info( void* h, int which, int32_t* out ) {
	const PackedWalk& walk = ( (const Run*) h )->walk[which];
	out[0] = (int32_t) walk.hotSlots;

	for( int k = 0; k < 8; k++ ) {
		out[1 + k] = walk.first[k];
	}
}

size_t rl_record_of( void* h, int which, const int** data ) {
	const PackedWalk& walk = ( (const Run*) h )->walk[which];
	*data = walk.recordOf.data();
	return walk.recordOf.size();
}

void rl_tables( void* h, uint64_t* out ) {
	const RelinkTables& t = ( (const Run*) h )->tables;
	out[0] = t.numLevels();
	out[1] = t.runs.size();
	out[2] = t.levelNodes.size();
	out[3] = t.bytes();
	out[4] = t.hotPerStream;
}

void rl_free( void* h ) {
	delete (Run*) h;
}

}  // extern "C"
