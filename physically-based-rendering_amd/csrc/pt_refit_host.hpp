// pt_refit_host.hpp — the host side of pbr_update_vertices (pbr_hip.hip; the kernels: pt_refit.hpp) that needs no device:
// whether a flat tree can be refitted at all, every node's parent, subtree end and height, its record in the reference-order
// stream, the cut of the tree into the pieces the kernels work on, and the refit itself in plain C++.
// Host code only, no HIP: tests/refit_driver.cpp builds it with a plain C++17 compiler (-ffp-contract=off, like the library's
// host code) and tests/refit_ref.py restates the fold in numpy.
//
// The boxes, operation by operation (include/pbr_hip.h, pbr_update_vertices), per component in binary32:
//   leaf       acc = corner a of its first face; then b, c, and the second face's a, b, c if there is one:
//              lo = ( v < lo ) ? v : lo, hi = ( v > hi ) ? v : hi
//   container  (node 0 included) the same fold over its children's boxes in depth-first child order, starting from the first
//              child's box; children of i: c0 = i + 1, c1 = end( c0 ), ... below end( i )
// Minimum and maximum are exact, so the order only decides between -0 and +0 — it is fixed all the same.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "pt_scene_pack.hpp"

// The cut: a maximal subtree of at most kRefitSubtree nodes is a contiguous index range [r, end( r )) and is refitted by one
// workgroup in LDS; consecutive such subtrees share a workgroup while they fit kRefitSubtree thread slots together.  The
// nodes above the cut — containers all — are refitted level by level, lowest first, by one more launch.
constexpr uint32_t kRefitSubtree = 256;
constexpr uint32_t kRefitNoNode = 0xFFFFFFFFu;

struct RefitPlan {
	bool nested = false;               // the verdict: every container's children tile [i + 1, end( i )) exactly
	std::string why;                   // ... and the reason when they do not
	std::vector<uint32_t> parent;      // per node (node 0: kRefitNoNode)
	std::vector<uint32_t> end;         // per node: where its subtree ends
	std::vector<uint32_t> height;      // per node: a leaf 0, a container 1 + its highest child's
	std::vector<int> recordOf;         // per node: its record in the reference-order stream (node 0: -1, it has none)

	// ---- the work partition ----
	uint32_t subtreeCap = kRefitSubtree;
	std::vector<uint32_t> subtreeRoots;   // the maximal subtrees of at most subtreeCap nodes, ascending
	std::vector<uint32_t> groupFirst;     // group g = subtreeRoots[groupFirst[g] .. groupFirst[g + 1]): one workgroup
	std::vector<uint32_t> slots;          // numGroups() x subtreeCap: the node of every thread slot, or kRefitNoNode
	std::vector<uint32_t> topNodes;       // the nodes above the cut, by height, then by index
	std::vector<uint32_t> topLevelFirst;  // level l = topNodes[topLevelFirst[l] .. topLevelFirst[l + 1])

	// ---- what the kernels read per node ----
	std::vector<uint32_t> info;           // a leaf: leafWord (bit 31 set); a container: end
	std::vector<uint16_t> height16;       // the height, for the nodes below the cut (above it: 0xFFFF, never read)

	uint32_t numGroups() const { return groupFirst.empty() ? 0u : (uint32_t) groupFirst.size() - 1u; }
	uint32_t numLevels() const { return topLevelFirst.empty() ? 0u : (uint32_t) topLevelFirst.size() - 1u; }
};

inline bool refitNotNested( RefitPlan* plan, const char* fmt, uint32_t a, uint32_t b, uint32_t c ) {
	char buf[256];
	std::snprintf( buf, sizeof( buf ), fmt, a, b, c );
	plan->nested = false;
	plan->why = buf;
	return false;
}

// Parent, end, height and the verdict.  checkScene accepts any forward link; a refit needs more: node 0 a container that
// spans the array, every subtree inside its parent's, no container without a child (it has no box to fold).
inline bool refitNesting( const SceneTree& tree, RefitPlan* plan ) {
	const uint32_t N = tree.size();
	plan->parent.assign( N, kRefitNoNode );
	plan->end.assign( N, 0 );
	plan->height.assign( N, 0 );
	plan->nested = true;
	plan->why.clear();

	if( N < 2 || tree.face0s[0] >= 0 ) {
		return refitNotNested( plan, "node 0 is not a container", 0, 0, 0 );
	}

	std::vector<uint32_t> open;

	for( uint32_t i = 0; i < N; i++ ) {
		while( !open.empty() && i >= plan->end[open.back()] ) {
			open.pop_back();
		}

		if( i > 0 && open.empty() ) {
			return refitNotNested( plan, "node %u lies outside node 0's subtree [1, %u)", i, plan->end[0], 0 );
		}

		const uint32_t up = open.empty() ? kRefitNoNode : open.back();
		const uint32_t upEnd = open.empty() ? N : plan->end[up];
		plan->parent[i] = up;

		if( tree.face0s[i] >= 0 ) {
			plan->end[i] = i + 1;
			continue;
		}

		plan->end[i] = ( tree.links[i] > (int) i ) ? (uint32_t) tree.links[i] : upEnd;

		if( plan->end[i] > upEnd ) {
			return refitNotNested( plan, "container %u: its miss link %u points past its parent's subtree, which ends at %u", i, plan->end[i], upEnd );
		}
		if( plan->end[i] <= i + 1 ) {
			return refitNotNested( plan, "container %u has no child: its subtree [%u, %u) is empty", i, i + 1, plan->end[i] );
		}

		open.push_back( i );
	}

	for( uint32_t i = N - 1; i > 0; i-- ) {   // children come behind their parent
		const uint32_t up = plan->parent[i];
		plan->height[up] = std::max( plan->height[up], plan->height[i] + 1 );
	}

	return true;
}

// The cut of a nested tree (refitNesting) for subtrees of at most `cap` nodes, and the kernels' tables.
inline void refitPartition( const SceneTree& tree, uint32_t cap, RefitPlan* plan ) {
	const uint32_t N = tree.size();
	plan->subtreeCap = cap;
	plan->subtreeRoots.clear();
	plan->topNodes.clear();

	for( uint32_t i = 0; i < N; ) {
		if( plan->end[i] - i <= cap ) {
			plan->subtreeRoots.push_back( i );
			i = plan->end[i];
		}
		else {
			plan->topNodes.push_back( i++ );
		}
	}

	plan->groupFirst.assign( 1, 0 );
	plan->slots.clear();
	uint32_t used = 0;

	for( uint32_t s = 0; s < plan->subtreeRoots.size(); s++ ) {
		const uint32_t root = plan->subtreeRoots[s], size = plan->end[root] - root;

		if( used + size > cap ) {
			plan->slots.resize( plan->slots.size() + ( cap - used ), kRefitNoNode );
			plan->groupFirst.push_back( s );
			used = 0;
		}

		for( uint32_t k = 0; k < size; k++ ) {
			plan->slots.push_back( root + k );
		}

		used += size;
	}

	plan->slots.resize( plan->slots.size() + ( cap - used ), kRefitNoNode );
	plan->groupFirst.push_back( (uint32_t) plan->subtreeRoots.size() );

	std::stable_sort( plan->topNodes.begin(), plan->topNodes.end(), [&]( uint32_t a, uint32_t b ) { return plan->height[a] < plan->height[b]; } );
	plan->topLevelFirst.clear();

	for( uint32_t k = 0; k < plan->topNodes.size(); k++ ) {
		if( k == 0 || plan->height[plan->topNodes[k]] != plan->height[plan->topNodes[k - 1]] ) {
			plan->topLevelFirst.push_back( k );
		}
	}

	plan->topLevelFirst.push_back( (uint32_t) plan->topNodes.size() );

	plan->info.resize( N );
	plan->height16.assign( N, 0xFFFF );

	for( uint32_t i = 0; i < N; i++ ) {
		plan->info[i] = ( tree.face0s[i] >= 0 ) ? (uint32_t) leafWord( tree, i ) : plan->end[i];
	}

	for( uint32_t node : plan->slots ) {
		if( node != kRefitNoNode ) {
			plan->height16[node] = (uint16_t) plan->height[node];   // below cap <= 65536 by the subtree's size
		}
	}
}

// Everything pbr_upload_scene keeps for pbr_update_vertices.  recordOf: of the reference-order stream (PackedWalk::recordOf).
inline void planRefit( const SceneTree& tree, const std::vector<int>& recordOf, uint32_t cap, RefitPlan* plan ) {
	plan->recordOf.assign( recordOf.begin(), recordOf.begin() + std::min<size_t>( recordOf.size(), tree.size() ) );

	if( refitNesting( tree, plan ) ) {
		refitPartition( tree, cap, plan );
	}
}

inline void refitFold( float lo[3], float hi[3], const float vLo[3], const float vHi[3] ) {
	for( int k = 0; k < 3; k++ ) {
		lo[k] = ( vLo[k] < lo[k] ) ? vLo[k] : lo[k];
		hi[k] = ( vHi[k] > hi[k] ) ? vHi[k] : hi[k];
	}
}

// A container's box: the fold over its children's boxes in `nodes`, depth-first child order, from the first child's.
inline void refitContainerBox( const RefitPlan& plan, const pbr_bvh_node* nodes, uint32_t i, float lo[3], float hi[3] ) {
	for( uint32_t c = i + 1; c < plan.end[i]; c = plan.end[c] ) {
		const float cLo[3] = { nodes[c].bbMin.x, nodes[c].bbMin.y, nodes[c].bbMin.z };
		const float cHi[3] = { nodes[c].bbMax.x, nodes[c].bbMax.y, nodes[c].bbMax.z };

		if( c == i + 1 ) {
			std::copy( cLo, cLo + 3, lo );
			std::copy( cHi, cHi + 3, hi );
		}
		else {
			refitFold( lo, hi, cLo, cHi );
		}
	}
}

inline void refitStoreBox( pbr_bvh_node* nodes, uint32_t i, const float lo[3], const float hi[3] ) {
	nodes[i].bbMin.x = lo[0];
	nodes[i].bbMin.y = lo[1];
	nodes[i].bbMin.z = lo[2];
	nodes[i].bbMax.x = hi[0];
	nodes[i].bbMax.y = hi[1];
	nodes[i].bbMax.z = hi[2];
}

// The refit in plain C++: the boxes of `nodes` (the tree's, N entries) from the vertices; the .w words stay.
inline void refitBoxes( const SceneTree& tree, const RefitPlan& plan, const pbr_uint4* facesV, const pbr_float4* vertices, pbr_bvh_node* nodes ) {
	const uint32_t N = tree.size();

	for( uint32_t i = N; i-- > 0; ) {   // children come behind their parent
		float lo[3], hi[3];

		if( tree.face0s[i] >= 0 ) {
			const int faces = ( tree.links[i] >= 0 ) ? 2 : 1;

			for( int f = 0; f < faces; f++ ) {
				const pbr_uint4& fv = facesV[tree.face0s[i] + f];
				const uint32_t corners[3] = { fv.x, fv.y, fv.z };

				for( int k = 0; k < 3; k++ ) {
					const pbr_float4& v = vertices[corners[k]];
					const float p[3] = { v.x, v.y, v.z };

					if( f == 0 && k == 0 ) {
						std::copy( p, p + 3, lo );
						std::copy( p, p + 3, hi );
					}
					else {
						refitFold( lo, hi, p, p );
					}
				}
			}
		}
		else {
			refitContainerBox( plan, nodes, i, lo, hi );
		}

		refitStoreBox( nodes, i, lo, hi );
	}
}

// Why pbr_update_vertices (or `call`: pbr_update_geometry takes its positions through here) refuses these vertices
// (PBR_EINVAL, the message in *why), or PBR_OK.
inline int checkRefitVertices( const pbr_float4* vertices, uint32_t num_vertices, uint32_t uploaded, std::string* why, const char* call = "pbr_update_vertices" ) {
	if( vertices == nullptr ) {
		return packFail( why, PBR_EINVAL, "%s: null vertices", call );
	}
	if( num_vertices != uploaded ) {
		return packFail( why, PBR_EINVAL, "%s: %u vertices, the uploaded scene has %u (the topology is kept)", call, num_vertices, uploaded );
	}

	for( uint32_t i = 0; i < num_vertices; i++ ) {
		const pbr_float4& v = vertices[i];

		if( !std::isfinite( v.x ) || !std::isfinite( v.y ) || !std::isfinite( v.z ) ) {
			return packFail( why, PBR_EINVAL, "%s: vertex %u is not finite", call, i );
		}
	}

	return PBR_OK;
}

// ... and why pbr_update_geometry refuses these normals.  NULL with num_normals == 0 keeps the context's normals; otherwise the
// count is the upload's and every x, y, z is finite (the fourth component is padding, as for a vertex).
inline int checkRefitNormals( const pbr_float4* normals, uint32_t num_normals, uint32_t uploaded, std::string* why ) {
	if( ( normals == nullptr ) != ( num_normals == 0 ) ) {
		return packFail( why, PBR_EINVAL, "pbr_update_geometry: %s normals with num_normals = %u (NULL and 0 keep the normals)", ( normals == nullptr ) ? "null" : "non-null", num_normals );
	}
	if( normals == nullptr ) {
		return PBR_OK;
	}
	if( num_normals != uploaded ) {
		return packFail( why, PBR_EINVAL, "pbr_update_geometry: %u normals, the uploaded scene has %u (the topology is kept)", num_normals, uploaded );
	}

	for( uint32_t i = 0; i < num_normals; i++ ) {
		const pbr_float4& n = normals[i];

		if( !std::isfinite( n.x ) || !std::isfinite( n.y ) || !std::isfinite( n.z ) ) {
			return packFail( why, PBR_EINVAL, "pbr_update_geometry: normal %u is not finite", i );
		}
	}

	return PBR_OK;
}
