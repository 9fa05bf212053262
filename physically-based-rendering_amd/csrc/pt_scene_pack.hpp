// pt_scene_pack.hpp — the caller's scene as the device buffers the kernels read (pbr_upload_scene, pbr_hip.hip): the checks
// of every index the kernels will follow, the hot-node ranking, the successor tables of the reference order and of the
// ray-ordered walks, the node records, and the face, Phong, material and light buffers.
// Host code only, no HIP: tests/scene_pack_driver.cpp builds it with a plain C++17 compiler and decodes what it packs.  The
// library's host code is built with -ffp-contract=off; so is the driver, so that the ranking comes out the same.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "pbr_hip.h"

// One 16-byte word of a device buffer (a float4 there).
struct Quad {
	float x, y, z, w;
};
static_assert( sizeof( Quad ) == 16, "a Quad is a float4 on the device" );

// What one block can stage in LDS with a CU's 160 KB to itself: the cap of the ranked prefix of every node stream, in bytes.
constexpr uint32_t kLdsStageBytes = 160 * 1024 - 256;

// A record reference is the record's byte offset in its stream (pt_kernel.hpp, Cursor): 31 bits.
constexpr size_t kRefLimit = (size_t) 1 << 31;

// The scene's flat tree as checkScene found it.
struct SceneTree {
	std::vector<pbr_bvh_node> bvh;
	std::vector<int> face0s, links;   // per node: first face or -1 (a container); second face / miss link
	std::vector<uint32_t> ranked;     // the nodes ranked for LDS staging, most visited first

	uint32_t size() const { return (uint32_t) bvh.size(); }
};

// The node records of one layout (pbr_config.traversal; 0: the reference order).  Layouts 1 - 3 start with 32 bytes of
// header, the eight first references, where firstNode() reads them; layout 0 has none.
struct PackedWalk {
	std::vector<Quad> storage;
	uint32_t hotSlots = 0;       // the ranked records at the head of the records, in 32-byte slots
	int first[8] = {};           // per order: the reference a ray starts at (layout 0: first[0], the record of node 1)
	std::vector<int> recordOf;   // per stream and node: its record (-1: none); the compact layout has one stream
};

struct PackedScene {
	PackedWalk nodes;            // the reference order's stream
	std::vector<Quad> tris, triPN, mats, lights;
};

inline int packFail( std::string* why, int code, const char* fmt, ... ) {
	char buf[512];
	va_list ap;
	va_start( ap, fmt );
	vsnprintf( buf, sizeof( buf ), fmt, ap );
	va_end( ap );

	if( why != nullptr ) {
		*why = buf;
	}

	return code;
}

inline float wordOf( int v ) {
	float f;
	std::memcpy( &f, &v, sizeof( f ) );
	return f;
}

// Is w an integer-valued float in [lo, hi]?
inline bool integral( float w, double lo, double hi ) {
	return ( w == std::floor( w ) ) && ( (double) w >= lo ) && ( (double) w <= hi );
}

// ---- hot nodes: rank by expected visit frequency ----
// A node is visited when its parent's box was hit, i.e. (for rays without preferred
// position) in proportion to the parent's surface area.  In the DFS array a container's
// subtree is [i + 1, escape) with escape = its miss link (or N), so parents fall out of one
// stack walk.  Measured against real visit histograms this ranking captures 56 % / 40 % /
// 18 % of all node visits with 1024 slots (Sponza- / Dragon-class / hairball), within 4
// points of the best possible choice.
// (The escape is not the ordered walk's subtree end, walkTables: this ranking is kept as it was measured.)
inline void rankHotNodes( SceneTree* tree ) {
	const uint32_t N = tree->size();
	std::vector<double> weight( N, 0.0 );
	{
		auto area = [&]( uint32_t i ) {
			const pbr_bvh_node& n = tree->bvh[i];
			const double dx = std::fabs( (double) n.bbMax.x - n.bbMin.x );
			const double dy = std::fabs( (double) n.bbMax.y - n.bbMin.y );
			const double dz = std::fabs( (double) n.bbMax.z - n.bbMin.z );
			return 2.0 * ( dx * dy + dz * dy + dx * dz );
		};
		std::vector<std::pair<uint32_t, double>> stack;   // (escape, area)
		const double rootArea = area( 0 );

		for( uint32_t i = 0; i < N; i++ ) {
			while( !stack.empty() && i >= stack.back().first ) {
				stack.pop_back();
			}

			weight[i] = stack.empty() ? rootArea : stack.back().second;

			if( tree->face0s[i] < 0 ) {
				const uint32_t escape = ( tree->links[i] > (int) i ) ? (uint32_t) tree->links[i] : N;
				stack.push_back( std::make_pair( escape, area( i ) ) );
			}
		}
	}

	std::vector<uint32_t>& ranked = tree->ranked;
	ranked.clear();
	ranked.reserve( N );

	for( uint32_t i = 1; i < N; i++ ) {   // node 0 (the root) is never fetched
		ranked.push_back( i );
	}

	const uint32_t numHot = (uint32_t) std::min<size_t>( ranked.size(), kLdsStageBytes / 32 );
	std::partial_sort( ranked.begin(), ranked.begin() + numHot, ranked.end(), [&]( uint32_t a, uint32_t b ) {
		return ( weight[a] != weight[b] ) ? ( weight[a] > weight[b] ) : ( a < b );
	} );
	ranked.resize( numHot );
}

// Everything pbr_upload_scene checks before it touches the device: every index the kernels will follow.
// tree (optional): the host copy of the checked tree, its hot nodes ranked.
inline int checkScene( const pbr_scene_desc* s, SceneTree* tree, std::string* why ) {
	if( s == nullptr || s->bvh == nullptr || s->facesV == nullptr || s->vertices == nullptr || s->materials == nullptr ) {
		return packFail( why, PBR_EINVAL, "scene: null array" );
	}
	if( s->num_nodes < 2 || s->num_faces == 0 || s->num_vertices == 0 || s->num_materials == 0 ) {
		return packFail( why, PBR_EINVAL, "scene: needs >= 2 BVH nodes (the root is never tested, pt_bvh.cl:84), faces, vertices and materials" );
	}
	if( s->brdf > 1 ) {
		return packFail( why, PBR_EINVAL, "scene: brdf must be 0 or 1" );
	}
	if( s->num_lights > 0 && s->lights == nullptr ) {
		return packFail( why, PBR_EINVAL, "scene: num_lights > 0 but lights is null" );
	}
	if( s->num_nodes > ( 1u << 24 ) || s->num_faces > ( 1u << 24 ) ) {
		return packFail( why, PBR_EINVAL, "scene: node / face indices are stored as floats and must stay below 2^24" );
	}

	// ---- nodes: validate every link the walk can follow ----
	std::vector<int> face0s( s->num_nodes ), links( s->num_nodes );

	for( uint32_t i = 0; i < s->num_nodes; i++ ) {
		const pbr_bvh_node& n = s->bvh[i];

		if( n.bbMin.w == -1.0f ) {
			// container node: miss link in [-1, N) (the walk stops outside (0, N), pt_bvh.cl:122)
			if( !integral( n.bbMax.w, -1.0, (double) s->num_nodes - 1.0 ) ) {
				return packFail( why, PBR_EINVAL, "node %u: miss link %g is not an index", i, (double) n.bbMax.w );
			}

			// ... and FORWARD: the stackless walk has no visited set, so a ray that keeps missing a box whose link
			// points at or before it would circle forever (the reference's flattening only emits links behind the
			// subtree, PathTracer.cpp:300-330; -1 and 0 end the walk)
			if( i > 0 && n.bbMax.w > 0.0f && n.bbMax.w <= (float) i ) {
				return packFail( why, PBR_EINVAL, "node %u: miss link %g must point forward (or be -1 / 0 = end of the walk)", i, (double) n.bbMax.w );
			}

			face0s[i] = -1;
			links[i] = (int) n.bbMax.w;
		}
		else if( integral( n.bbMin.w, 0.0, (double) s->num_faces - 1.0 ) ) {
			// leaf: the second face, if any, is the next one in leaf order (PathTracer.cpp:267-268)
			if( !( n.bbMax.w == -1.0f || n.bbMax.w == n.bbMin.w + 1.0f ) || n.bbMax.w > (float) ( s->num_faces - 1 ) ) {
				return packFail( why, PBR_EINVAL, "node %u: second face %g is neither -1 nor first face + 1", i, (double) n.bbMax.w );
			}

			face0s[i] = (int) n.bbMin.w;
			links[i] = (int) n.bbMax.w;
		}
		else {
			return packFail( why, PBR_EINVAL, "node %u: bbMin.w = %g is neither -1 nor a face index", i, (double) n.bbMin.w );
		}
	}

	if( face0s[s->num_nodes - 1] < 0 ) {
		return packFail( why, PBR_EINVAL, "node %u: the last node is a container (its children would lie outside the array)", s->num_nodes - 1 );
	}

	// ---- faces ----
	for( uint32_t f = 0; f < s->num_faces; f++ ) {
		const pbr_uint4& fv = s->facesV[f];

		if( fv.x >= s->num_vertices || fv.y >= s->num_vertices || fv.z >= s->num_vertices ) {
			return packFail( why, PBR_EINVAL, "face %u: vertex index out of range", f );
		}
		if( fv.w >= s->num_materials ) {
			return packFail( why, PBR_EINVAL, "face %u: material index %u out of range (faces without usemtl carry -1)", f, fv.w );
		}
	}

	if( tree != nullptr ) {
		tree->bvh.assign( s->bvh, s->bvh + s->num_nodes );
		tree->face0s.swap( face0s );
		tree->links.swap( links );
		rankHotNodes( tree );
	}

	return PBR_OK;
}

// ---- the successor tables (pbr_config.traversal, include/pbr_hip.h) ----------------------------------------------------
// Per order k and node i: onHit[k * N + i], where a ray goes when container i's box is hit, and onNext[k * N + i], where it
// goes otherwise (a missed container, every leaf); -1: the walk ends.
//
// The reference order (layout 0): a hit continues at index + 1, a miss at the container's link (pt_bvh.cl:102,112; the child
// with the bigger surface area sits at index + 1, accelstructures/BVH.cpp:335-343), a leaf at index + 1; the walk stops
// outside (0, N), pt_bvh.cl:122.
//
// The ray-ordered walk is not a reference structure.  The records of the node stream name their successors explicitly
// (pt_kernel.hpp, decodeNode), so another visiting order is another set of successor words over the same boxes and leaf
// words — the kernels do not change, a walk only starts somewhere else.
//
// The tree behind the flat array: a leaf ends at index + 1, a container i at its miss link when that is > i, else where
// its parent ends (the root: N); its children are c0 = i + 1, c1 = end( c0 ), ... below end( i ) — the flattening drops
// nodes (PathTracer.cpp:250-256), so there can be more than two.
// A child's key on an axis: bbMin[axis] + bbMax[axis] (binary32).  A container's children in an order = the DFS child
// list insertion-sorted — a child moves in front of its predecessor while its key is smaller (ascending) / greater
// (descending); as an algorithm, so that ties and NaN keys have one outcome.
//   scheme 1, six orders   order 2 * a + neg sorts EVERY container on axis a, descending when neg; a ray takes the order of
//                          its direction's dominant axis and that component's sign (walkOrderOf, pt_kernel.hpp)
//   scheme 2, eight orders order k = sign bits of the direction; a container sorts on ITS axis — the one its children's keys
//                          spread furthest on (max - min, x before y before z on ties) — descending when that bit of k is set
// Successors in an order: a hit container continues at its first child; child j's next is child j + 1, the last child's
// is its parent's next, the root's is "end"; a missed container and every leaf continue at next.
// Layout 3 = scheme 2's eight orders in the compact record (pt_kernel.hpp, "the compact record"): the successors are the same.
struct WalkTables {
	int K = 1;
	std::vector<int> onHit, onNext;
	std::vector<unsigned char> axisOf;   // layout 3: the axis a container sorts its children on
};

inline int walkTables( const SceneTree& tree, uint32_t layout, WalkTables* t, std::string* why ) {
	const bool compact = ( layout == PBR_WALK_EIGHT_ORDERS_COMPACT );
	const uint32_t scheme = compact ? 2u : layout;
	const int K = ( scheme == 0 ) ? 1 : ( scheme == 1 ) ? 6 : 8;
	const uint32_t N = tree.size();
	const std::vector<int>& face0s = tree.face0s;
	std::vector<int>& onHit = t->onHit;
	std::vector<int>& onNext = t->onNext;
	t->K = K;
	onHit.assign( (size_t) K * N, -1 );
	onNext.assign( (size_t) K * N, -1 );
	t->axisOf.assign( compact ? N : 0, 0 );

	if( scheme == 0 ) {
		for( uint32_t i = 0; i < N; i++ ) {
			onHit[i] = ( i + 1 < N ) ? (int) i + 1 : -1;
			onNext[i] = ( face0s[i] >= 0 ) ? onHit[i] : ( tree.links[i] > 0 ) ? tree.links[i] : -1;
		}
	}
	else {
		// where every subtree ends
		std::vector<uint32_t> end( N );
		{
			std::vector<uint32_t> open;

			for( uint32_t i = 0; i < N; i++ ) {
				while( !open.empty() && i >= end[open.back()] ) {
					open.pop_back();
				}

				if( face0s[i] >= 0 ) {
					end[i] = i + 1;
				}
				else {
					end[i] = ( tree.links[i] > (int) i ) ? (uint32_t) tree.links[i] : ( open.empty() ? N : end[open.back()] );
					open.push_back( i );
				}
			}
		}

		auto key = [&]( uint32_t node, int axis ) {
			const pbr_bvh_node& n = tree.bvh[node];
			return ( axis == 0 ) ? n.bbMin.x + n.bbMax.x : ( axis == 1 ) ? n.bbMin.y + n.bbMax.y : n.bbMin.z + n.bbMax.z;
		};

		std::vector<uint32_t> children, inOrder;

		for( uint32_t i = 0; i < N; i++ ) {
			if( face0s[i] >= 0 ) {
				continue;
			}

			children.clear();

			for( uint32_t c = i + 1; c < end[i]; c = end[c] ) {
				children.push_back( c );
			}

			int ownAxis = 0;

			if( scheme == 2 ) {
				float widest = -1.0f;

				for( int axis = 0; axis < 3; axis++ ) {
					float lo = INFINITY, hi = -INFINITY;

					for( uint32_t c : children ) {
						const float k = key( c, axis );
						lo = ( k < lo ) ? k : lo;
						hi = ( k > hi ) ? k : hi;
					}

					if( hi - lo > widest ) {
						widest = hi - lo;
						ownAxis = axis;
					}
				}
			}

			if( compact ) {
				t->axisOf[i] = (unsigned char) ownAxis;

				if( children.empty() ) {
					return packFail( why, PBR_EINVAL, "ray-ordered walk, compact records: container %u has no child (a record names its two first children)", i );
				}
			}

			for( int k = 0; k < K; k++ ) {
				const int axis = ( scheme == 1 ) ? k / 2 : ownAxis;
				const bool descending = ( scheme == 1 ) ? ( k & 1 ) != 0 : ( ( k >> ownAxis ) & 1 ) != 0;
				inOrder.clear();

				for( uint32_t c : children ) {
					const float mine = key( c, axis );
					size_t at = inOrder.size();
					inOrder.push_back( c );

					while( at > 0 ) {
						const float before = key( inOrder[at - 1], axis );

						if( !( descending ? ( mine > before ) : ( mine < before ) ) ) {
							break;
						}

						inOrder[at] = inOrder[at - 1];
						at--;
					}

					inOrder[at] = c;
				}

				const size_t base = (size_t) k * N;
				const int next = ( i == 0 ) ? -1 : onNext[base + i];   // written when i's parent was handled (parents come first)
				onHit[base + i] = inOrder.empty() ? next : (int) inOrder[0];

				for( size_t j = 0; j < inOrder.size(); j++ ) {
					onNext[base + inOrder[j]] = ( j + 1 < inOrder.size() ) ? (int) inOrder[j + 1] : next;
				}
			}
		}
	}

	for( int k = 0; k < K; k++ ) {      // every order must reach every node (a tree that is not properly nested fails here)
		const size_t base = (size_t) k * N;
		size_t seen = 0;

		for( int node = onHit[base]; node > 0; node = ( face0s[node] < 0 ) ? onHit[base + node] : onNext[base + node] ) {
			if( ++seen >= N ) {
				return packFail( why, PBR_ESTATE, "ray-ordered walk: order %d does not visit every node once", k );
			}
		}

		if( seen != N - 1 ) {
			return packFail( why, PBR_ESTATE, "ray-ordered walk: order %d reaches %zu of %u nodes", k, seen, N - 1 );
		}
	}

	return PBR_OK;
}

// Records: [ the ranked nodes, rank by rank, all streams of a rank next to each other (any prefix a block stages in LDS
// serves every order alike) ][ stream 0's other nodes in its order's depth-first sequence ][ stream 1's ] ...  The reference
// order's sequence is the array's (a cold node's hit successor is the adjacent record; any order is legal — every record
// names its successors.  Treelets, a connected piece of the tree per 128-byte line, were built and measured in round 3:
// -13 ... -19 % distinct lines per ray offline, +0.0 / +0.2 / +0.7 % on the GPU; lab/src/node_stream_treelets.txt.)
// Returns the number of records placed.
inline size_t placeRecords( const SceneTree& tree, const WalkTables& t, int streams, uint32_t hotPerStream, std::vector<int>* recordOf ) {
	const uint32_t N = tree.size();
	recordOf->assign( (size_t) streams * N, -1 );
	size_t nextRecord = 0;

	for( uint32_t r = 0; r < hotPerStream; r++ ) {
		for( int k = 0; k < streams; k++ ) {
			( *recordOf )[(size_t) k * N + tree.ranked[r]] = (int) nextRecord++;
		}
	}

	for( int k = 0; k < streams; k++ ) {
		const size_t base = (size_t) k * N;

		for( int node = t.onHit[base]; node > 0; node = ( tree.face0s[node] < 0 ) ? t.onHit[base + node] : t.onNext[base + node] ) {
			if( ( *recordOf )[base + node] < 0 ) {
				( *recordOf )[base + node] = (int) nextRecord++;
			}
		}
	}

	return nextRecord;
}

// a leaf's first word (pt_kernel.hpp, leafFace0 / leafFace1): its first face, and whether it has a second
inline int leafWord( const SceneTree& tree, uint32_t i ) {
	return (int) ( 0x80000000u | ( ( tree.links[i] >= 0 ) ? 0x40000000u : 0u ) | (uint32_t) tree.face0s[i] );
}

// The 32-byte record (pt_kernel.hpp, decodeNode): the box, then a container's hit and next references or a leaf's word and
// next reference; one stream per order.  first[k]: order k's reference of the node the walk starts at.
inline void encodeRecords32( const SceneTree& tree, const WalkTables& t, const std::vector<int>& recordOf, Quad* records, int* first ) {
	const uint32_t N = tree.size();

	for( int k = 0; k < t.K; k++ ) {
		const size_t base = (size_t) k * N;
		auto refOf = [&]( int node ) { return ( node > 0 ) ? recordOf[base + (size_t) node] * 32 : -1; };

		for( uint32_t i = 1; i < N; i++ ) {
			const pbr_bvh_node& n = tree.bvh[i];
			const int w0 = ( tree.face0s[i] < 0 ) ? refOf( t.onHit[base + i] ) : leafWord( tree, i );
			const int w1 = refOf( t.onNext[base + i] );
			Quad* rec = records + (size_t) recordOf[base + i] * 2;
			rec[0] = Quad { n.bbMin.x, n.bbMin.y, n.bbMax.x, n.bbMax.y };
			rec[1] = Quad { n.bbMin.z, n.bbMax.z, wordOf( w0 ), wordOf( w1 ) };
		}

		first[k] = refOf( t.onHit[base] );
	}
}

// The compact 64-byte record of the eight-order walk (pt_kernel.hpp, "the compact record"): the box, two hit candidates —
// order 0's (every container ascending) and order 7's (every container descending), the latter with the container's axis
// bit — or the leaf word, then the eight orders' next references.  One stream; order 0's depth-first sequence follows the
// ranked nodes, so that a hit container's ascending first child is the adjacent record.
inline void encodeCompactRecords( const SceneTree& tree, const WalkTables& t, const std::vector<int>& recordOf, Quad* records, int* first ) {
	const uint32_t N = tree.size();
	auto refOf = [&]( int node ) { return ( node > 0 ) ? recordOf[(size_t) node] * 64 : -1; };

	for( uint32_t i = 1; i < N; i++ ) {
		const pbr_bvh_node& n = tree.bvh[i];
		const bool leaf = ( tree.face0s[i] >= 0 );
		const int h0 = leaf ? leafWord( tree, i ) : refOf( t.onHit[i] );
		const int h1 = leaf ? 0 : refOf( t.onHit[(size_t) 7 * N + i] ) | ( 4 << t.axisOf[i] );
		int next[8];

		for( int k = 0; k < 8; k++ ) {
			next[k] = refOf( t.onNext[(size_t) k * N + i] );
		}

		Quad* rec = records + (size_t) recordOf[i] * 4;
		rec[0] = Quad { n.bbMin.x, n.bbMin.y, n.bbMax.x, n.bbMax.y };
		rec[1] = Quad { n.bbMin.z, n.bbMax.z, wordOf( h0 ), wordOf( h1 ) };
		rec[2] = Quad { wordOf( next[0] ), wordOf( next[1] ), wordOf( next[2] ), wordOf( next[3] ) };
		rec[3] = Quad { wordOf( next[4] ), wordOf( next[5] ), wordOf( next[6] ), wordOf( next[7] ) };
	}

	for( int k = 0; k < 8; k++ ) {
		first[k] = refOf( t.onHit[(size_t) k * N] );
	}
}

// The node records of a layout: 0 the reference order, 1 six orders, 2 eight orders, 3 eight orders in compact records.
inline int packWalk( const SceneTree& tree, uint32_t layout, PackedWalk* out, std::string* why ) {
	const bool compact = ( layout == PBR_WALK_EIGHT_ORDERS_COMPACT );
	const int K = ( layout == 0 ) ? 1 : ( layout == 1 ) ? 6 : 8;
	const int streams = compact ? 1 : K;
	const size_t recordBytes = compact ? 64 : 32;
	const uint32_t N = tree.size();

	if( N < 2 ) {
		return packFail( why, PBR_ESTATE, "ray-ordered walk: no host copy of the scene's tree" );
	}
	if( (size_t) streams * N * recordBytes >= kRefLimit ) {
		return ( layout == 0 ) ? packFail( why, PBR_EINVAL, "upload_scene: the node stream would exceed 2 GiB (record references are 31-bit byte offsets)" )
		       : compact ? packFail( why, PBR_EINVAL, "ray-ordered walk: %u compact records exceed 2 GiB (record references are 31-bit byte offsets)", N )
		       : packFail( why, PBR_EINVAL, "ray-ordered walk: %d streams of %u records exceed 2 GiB (record references are 31-bit byte offsets); traversal = PBR_WALK_EIGHT_ORDERS_COMPACT holds 2^24 nodes", K, N );
	}

	WalkTables t;
	const int status = walkTables( tree, layout, &t, why );

	if( status != PBR_OK ) {
		return status;
	}

	const uint32_t hotPerStream = (uint32_t) std::min<size_t>( tree.ranked.size(), kLdsStageBytes / ( recordBytes * (size_t) streams ) );
	const size_t numRecords = placeRecords( tree, t, streams, hotPerStream, &out->recordOf ) + 1;   // + 1 record of padding
	const size_t header = ( layout == 0 ) ? 0 : 2;
	out->storage.assign( header + numRecords * ( recordBytes / sizeof( Quad ) ), Quad { 0.0f, 0.0f, 0.0f, 0.0f } );
	out->hotSlots = hotPerStream * (uint32_t) streams * (uint32_t) ( recordBytes / 32 );   // 32-byte slots are the unit of a plan's LDS share

	if( compact ) {
		encodeCompactRecords( tree, t, out->recordOf, out->storage.data() + header, out->first );
	}
	else {
		encodeRecords32( tree, t, out->recordOf, out->storage.data() + header, out->first );
	}

	for( int k = K; k < 8; k++ ) {
		out->first[k] = out->first[0];
	}

	if( header != 0 ) {
		std::memcpy( out->storage.data(), out->first, sizeof( out->first ) );
	}

	return PBR_OK;
}

// Everything pbr_upload_scene puts on the device for a checked scene, but the ray-ordered walk's streams.
inline int packScene( const pbr_scene_desc* s, const SceneTree& tree, PackedScene* out, std::string* why ) {
	const int status = packWalk( tree, 0, &out->nodes, why );

	if( status != PBR_OK ) {
		return status;
	}

	// ---- faces: gather the corners; store a, b - a, c - a (what pt_intersect.cl:98-99 computes) ----
	std::vector<Quad>& tris = out->tris;
	tris.assign( (size_t) ( s->num_faces + 1 ) * 3, Quad { 0.0f, 0.0f, 0.0f, 0.0f } );   // + 1: testLeaf reads face + 1 ahead

	for( uint32_t f = 0; f < s->num_faces; f++ ) {
		const pbr_uint4& fv = s->facesV[f];

		const pbr_float4& a = s->vertices[fv.x];
		const pbr_float4& b = s->vertices[fv.y];
		const pbr_float4& c = s->vertices[fv.z];
		const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
		const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
		const int material = (int) fv.w;

		tris[(size_t) f * 3 + 0] = Quad { a.x, a.y, a.z, e1x };
		tris[(size_t) f * 3 + 1] = Quad { e1y, e1z, e2x, e2y };
		tris[(size_t) f * 3 + 2] = Quad { e2z, wordOf( material ), 0.0f, 0.0f };
	}

	// ---- Phong tessellation input: the exact corners and their vertex normals, gathered per face ----
	// (pt_intersect.cl:146-157 gathers them through facesV / facesN per test).  The default flat test never reads
	// facesN, so scenes whose normal indices are unusable stay valid; they just cannot be configured with PHONGTESS.
	bool usable = ( s->facesN != nullptr && s->normals != nullptr && s->num_normals > 0 );

	for( uint32_t f = 0; usable && f < s->num_faces; f++ ) {
		const pbr_uint4& fn = s->facesN[f];
		usable = ( fn.x < s->num_normals && fn.y < s->num_normals && fn.z < s->num_normals );
	}

	out->triPN.assign( usable ? (size_t) s->num_faces * 6 : 0, Quad { 0.0f, 0.0f, 0.0f, 0.0f } );

	for( uint32_t f = 0; usable && f < s->num_faces; f++ ) {
		const pbr_uint4& fv = s->facesV[f];
		const pbr_uint4& fn = s->facesN[f];
		const uint32_t vi[3] = { fv.x, fv.y, fv.z }, ni[3] = { fn.x, fn.y, fn.z };

		for( int k = 0; k < 3; k++ ) {
			const pbr_float4& v = s->vertices[vi[k]];
			const pbr_float4& n = s->normals[ni[k]];
			out->triPN[(size_t) f * 6 + k] = Quad { v.x, v.y, v.z, 0.0f };
			out->triPN[(size_t) f * 6 + 3 + k] = Quad { n.x, n.y, n.z, 0.0f };
		}
	}

	// ---- materials: one 64-byte shape for both BRDFs ----
	std::vector<Quad>& mats = out->mats;
	mats.assign( (size_t) s->num_materials * 4, Quad { 0.0f, 0.0f, 0.0f, 0.0f } );

	for( uint32_t i = 0; i < s->num_materials; i++ ) {
		if( s->brdf == 0 ) {
			const pbr_material_schlick& m = ( (const pbr_material_schlick*) s->materials )[i];
			mats[(size_t) i * 4 + 0] = Quad { m.data[0], m.data[1], m.data[2], m.data[3] };
			mats[(size_t) i * 4 + 2] = Quad { m.rgbDiff.x, m.rgbDiff.y, m.rgbDiff.z, 0.0f };
			mats[(size_t) i * 4 + 3] = Quad { m.rgbSpec.x, m.rgbSpec.y, m.rgbSpec.z, 0.0f };
		}
		else {
			const pbr_material_sa& m = ( (const pbr_material_sa*) s->materials )[i];
			mats[(size_t) i * 4 + 0] = Quad { m.data[0], m.data[1], m.data[2], m.data[3] };
			mats[(size_t) i * 4 + 1] = Quad { m.data[4], m.data[5], 0.0f, 0.0f };
			mats[(size_t) i * 4 + 2] = Quad { m.rgbDiff.x, m.rgbDiff.y, m.rgbDiff.z, 0.0f };
			mats[(size_t) i * 4 + 3] = Quad { m.rgbSpec.x, m.rgbSpec.y, m.rgbSpec.z, 0.0f };
		}
	}

	const uint32_t lightSlots = ( s->num_lights > 0 ) ? s->num_lights : 1;
	out->lights.assign( (size_t) lightSlots * 3, Quad { 0.0f, 0.0f, 0.0f, 0.0f } );

	for( uint32_t i = 0; i < s->num_lights; i++ ) {
		const pbr_light& l = s->lights[i];
		out->lights[(size_t) i * 3 + 0] = Quad { l.pos.x, l.pos.y, l.pos.z, l.pos.w };
		out->lights[(size_t) i * 3 + 1] = Quad { l.rgb.x, l.rgb.y, l.rgb.z, l.rgb.w };
		out->lights[(size_t) i * 3 + 2] = Quad { l.data.x, l.data.y, l.data.z, l.data.w };
	}

	return PBR_OK;
}
