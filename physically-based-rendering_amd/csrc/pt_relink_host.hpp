// pt_relink_host.hpp — pbr_update_vertices under a ray-ordered walk (pbr_refit_ordered_walk, include/pbr_hip.h): after the
// refit, the configured layout's records are rebuilt from the refitted boxes — packWalk's bytes (pt_scene_pack.hpp) without
// walkTables, placeRecords or the encoders, in three steps that need nothing but the tree's static shape, the hot-node
// ranking of the upload and the boxes in the reference-order stream:
//
//   sort     per container (node 0 included): its axis, and its depth-first child list insertion-sorted ascending and descending
//            (scheme 1: on every axis, six lists) into a table of N - 1 entries per list — every node but node 0 is one
//            container's child, so container i's lists start at childBase[i] = the number of children of the containers before it
//   levels   top-down by depth, per (container, order k): every child's `next` in order k (the following child of k's list, the
//            last one's is the container's own next, node 0's is "end"), and every child's pos = the number of cold records
//            in front of it in order k's depth-first sequence:
//                pos( child j ) = pos( i ) + ( i is cold and not node 0 ? 1 : 0 ) + sum of cold( child m ) over m < j in k's list
//            with cold( n ) = the non-hot nodes in [n, end( n )), a difference of a static prefix sum
//   records  per (node, order): the record in the layout's format — the box words as they stand in the reference-order stream, a
//            container's hit reference(s) = its first child in the order, its next reference(s); node n's record in stream k is
//                hot:  rank( n ) * streams + k          cold:  hotPerStream * streams + k * ( N - 1 - hotPerStream ) + pos
//            and the 32-byte header of eight first references
//
// The per-item bodies below (relinkSort, relinkLevel, relinkRecord32, relinkRecordCompact, relinkHeader) are what the kernels of
// pt_relink.hpp run, one item per thread; relinkWalk runs the same bodies in plain loops in the launches' order.  They are
// additions, subtractions, compares and integer work: nothing contracts, and the library's device and host code are built with
// -ffp-contract=off anyway.
// Host code only, no HIP: tests/relink_driver.cpp builds it with a plain C++17 compiler and compares relinkWalk with packWalk.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pt_refit_host.hpp"

#if defined( __HIPCC__ )
#define RELINK_FN __host__ __device__ inline
#define RELINK_ALIGN alignas( 16 )
#else
#define RELINK_FN inline
#define RELINK_ALIGN
#endif

// Loops over a container's children advance through the array, so they end by themselves; PBR_GUARD builds count them all the same.
#ifdef PBR_GUARD
#define RELINK_TRIP( trips, limit ) if( ++( trips ) > ( limit ) ) break
#else
#define RELINK_TRIP( trips, limit ) (void) ( trips )
#endif

constexpr uint32_t kRelinkCold = 0xFFFFFFFFu;   // rankOf: not among the layout's hot nodes
constexpr uint32_t kRelinkNarrow = 4096;        // a level of at most this many (container, order) items shares a one-workgroup launch with its neighbours
constexpr uint32_t kRelinkWideThreads = 256, kRelinkNarrowThreads = 1024;

struct RELINK_ALIGN RelinkQuad {
	float x, y, z, w;
};
static_assert( sizeof( RelinkQuad ) == sizeof( Quad ), "a RelinkQuad is a Quad" );

// What every step sees: the sizes, the static tables, the working tables and the streams.
struct RelinkView {
	uint32_t N, scheme, compact, K, V, streams, hotPerStream;
	// static, of the upload
	const RelinkQuad* refNodes;     // the reference-order stream: the refitted boxes
	const int* refRecordOf;         // node -> its record there
	const uint32_t* info;           // a leaf: leafWord (bit 31 set); a container: end (RefitPlan::info)
	const uint32_t* rankOf;         // node -> rank among the layout's hot nodes, or kRelinkCold
	const uint32_t* coldBefore;     // N + 1: the cold nodes among [1, n)
	const uint32_t* childBase;      // container -> where its child lists start
	// working tables
	unsigned char* axis;            // container -> the axis it sorts on (scheme 2)
	uint32_t* perm;                 // V x ( N - 1 ): the sorted child lists
	int* next;                      // K x N: order k's next node, -1: the walk ends
	uint32_t* pos;                  // streams x N
	// the configured layout's buffer
	int* header;                    // eight first references
	RelinkQuad* records;            // behind the header
};

RELINK_FN uint32_t relinkEnd( const RelinkView& v, uint32_t node ) {
	const uint32_t w = v.info[node];
	return ( w & 0x80000000u ) ? node + 1u : w;
}

RELINK_FN float relinkKey( const RelinkView& v, uint32_t node, int axis ) {
	const RelinkQuad* rec = v.refNodes + (size_t) v.refRecordOf[node] * 2;
	const RelinkQuad q0 = rec[0];

	if( axis == 0 ) {
		return q0.x + q0.z;
	}
	if( axis == 1 ) {
		return q0.y + q0.w;
	}

	const RelinkQuad q1 = rec[1];
	return q1.x + q1.y;
}

// Step 1, per container i.
RELINK_FN void relinkSort( const RelinkView& v, uint32_t i ) {
	const uint32_t end = v.info[i];
	int ownAxis = 0;
	uint32_t trips = 0;

	if( v.scheme == 2 ) {
		float widest = -1.0f;

		for( int axis = 0; axis < 3; axis++ ) {
			float lo = __builtin_inff(), hi = -__builtin_inff();

			for( uint32_t c = i + 1; c < end; c = relinkEnd( v, c ) ) {
				const float k = relinkKey( v, c, axis );
				lo = ( k < lo ) ? k : lo;
				hi = ( k > hi ) ? k : hi;
				RELINK_TRIP( trips, 3u * v.N );
			}

			if( hi - lo > widest ) {
				widest = hi - lo;
				ownAxis = axis;
			}
		}
	}

	v.axis[i] = (unsigned char) ownAxis;

	for( uint32_t variant = 0; variant < v.V; variant++ ) {
		const int axis = ( v.scheme == 1 ) ? (int) ( variant / 2u ) : ownAxis;
		const bool descending = ( variant & 1u ) != 0;
		uint32_t* list = v.perm + (size_t) variant * ( v.N - 1 ) + v.childBase[i];
		uint32_t count = 0;
		trips = 0;

		for( uint32_t c = i + 1; c < end; c = relinkEnd( v, c ) ) {
			const float mine = relinkKey( v, c, axis );
			uint32_t at = count++;

			while( at > 0 ) {
				const float before = relinkKey( v, list[at - 1], axis );

				if( !( descending ? ( mine > before ) : ( mine < before ) ) ) {
					break;
				}

				list[at] = list[at - 1];
				at--;
			}

			list[at] = c;
			RELINK_TRIP( trips, v.N );
		}
	}
}

// The list container i's children take in order k.
RELINK_FN const uint32_t* relinkList( const RelinkView& v, uint32_t i, uint32_t k ) {
	const uint32_t variant = ( v.scheme == 1 ) ? k : ( ( k >> v.axis[i] ) & 1u );
	return v.perm + (size_t) variant * ( v.N - 1 ) + v.childBase[i];
}

// Step 2, per (container i, order k); i's own next and pos were written by the level above.
RELINK_FN void relinkLevel( const RelinkView& v, uint32_t i, uint32_t k ) {
	const uint32_t end = v.info[i];
	const uint32_t* list = relinkList( v, i, k );
	const size_t base = (size_t) k * v.N;
	const bool placed = ( k < v.streams );
	const int myNext = ( i == 0 ) ? -1 : v.next[base + i];
	uint32_t p = ( i == 0 || !placed ) ? 0u : v.pos[base + i] + ( ( v.rankOf[i] == kRelinkCold ) ? 1u : 0u );
	uint32_t previous = 0, j = 0, trips = 0;

	for( uint32_t c = i + 1; c < end; c = relinkEnd( v, c ), j++ ) {
		const uint32_t child = list[j];

		if( j > 0 ) {
			v.next[base + previous] = (int) child;
		}
		if( placed ) {
			v.pos[base + child] = p;
			p += v.coldBefore[relinkEnd( v, child )] - v.coldBefore[child];
		}

		previous = child;
		RELINK_TRIP( trips, v.N );
	}

	v.next[base + previous] = myNext;   // a container has a child (refitNesting)
}

// node's record in stream k, in records
RELINK_FN uint32_t relinkRecordOf( const RelinkView& v, uint32_t node, uint32_t k ) {
	const uint32_t rank = v.rankOf[node];
	return ( rank != kRelinkCold ) ? rank * v.streams + k
	                               : v.hotPerStream * v.streams + k * ( v.N - 1u - v.hotPerStream ) + v.pos[(size_t) k * v.N + node];
}

RELINK_FN int relinkRef( const RelinkView& v, int node, uint32_t k ) {
	return ( node > 0 ) ? (int) ( relinkRecordOf( v, (uint32_t) node, k ) * ( v.compact ? 64u : 32u ) ) : -1;
}

RELINK_FN float relinkWord( int w ) {
	float f;
	__builtin_memcpy( &f, &w, sizeof( f ) );
	return f;
}

// Step 3, the 32-byte record of node n >= 1 in stream k (pt_scene_pack.hpp, encodeRecords32).
RELINK_FN void relinkRecord32( const RelinkView& v, uint32_t n, uint32_t k ) {
	const RelinkQuad* src = v.refNodes + (size_t) v.refRecordOf[n] * 2;
	const uint32_t word = v.info[n];
	const int w0 = ( word & 0x80000000u ) ? (int) word : relinkRef( v, (int) relinkList( v, n, k )[0], k );
	const int w1 = relinkRef( v, v.next[(size_t) k * v.N + n], k );
	const RelinkQuad q0 = src[0], q1 = src[1];
	RelinkQuad* rec = v.records + (size_t) relinkRecordOf( v, n, k ) * 2;
	rec[0] = q0;
	rec[1] = RelinkQuad { q1.x, q1.y, relinkWord( w0 ), relinkWord( w1 ) };
}

// Step 3, the compact 64-byte record of node n >= 1 (encodeCompactRecords): one stream, placed along order 0.
RELINK_FN void relinkRecordCompact( const RelinkView& v, uint32_t n ) {
	const RelinkQuad* src = v.refNodes + (size_t) v.refRecordOf[n] * 2;
	const uint32_t word = v.info[n];
	const bool leaf = ( word & 0x80000000u ) != 0;
	const int h0 = leaf ? (int) word : relinkRef( v, (int) relinkList( v, n, 0 )[0], 0 );
	const int h1 = leaf ? 0 : ( relinkRef( v, (int) relinkList( v, n, 7 )[0], 0 ) | ( 4 << v.axis[n] ) );
	int next[8];

	for( uint32_t k = 0; k < 8; k++ ) {
		next[k] = relinkRef( v, v.next[(size_t) k * v.N + n], 0 );
	}

	const RelinkQuad q0 = src[0], q1 = src[1];
	RelinkQuad* rec = v.records + (size_t) relinkRecordOf( v, n, 0 ) * 4;
	rec[0] = q0;
	rec[1] = RelinkQuad { q1.x, q1.y, relinkWord( h0 ), relinkWord( h1 ) };
	rec[2] = RelinkQuad { relinkWord( next[0] ), relinkWord( next[1] ), relinkWord( next[2] ), relinkWord( next[3] ) };
	rec[3] = RelinkQuad { relinkWord( next[4] ), relinkWord( next[5] ), relinkWord( next[6] ), relinkWord( next[7] ) };
}

// Step 3, once: the eight first references — node 0's first child per order; the orders a scheme does not have take order 0's.
RELINK_FN void relinkHeader( const RelinkView& v ) {
	for( uint32_t k = 0; k < 8; k++ ) {
		const uint32_t order = ( k < v.K ) ? k : 0u;
		v.header[k] = relinkRef( v, (int) relinkList( v, 0, order )[0], v.compact ? 0u : order );
	}
}

// ---- the static tables --------------------------------------------------------------------------------------------------

// One launch of the levels kernel: levels [firstLevel, firstLevel + numLevels) by `blocks` workgroups of `threads`; more than one
// level only with one workgroup, whose barrier separates them.
struct RelinkRun {
	uint32_t firstLevel, numLevels, blocks, threads;
};

struct RelinkTables {
	uint32_t layout = 0, N = 0, scheme = 0, compact = 0, K = 0, V = 0, streams = 0, hotPerStream = 0, hotSlots = 0;
	size_t recordBytes = 0, storageQuads = 0;     // of the layout's buffer, header and padding record included
	std::vector<uint32_t> rankOf, coldBefore, childBase;
	std::vector<uint32_t> levelNodes;             // the containers by depth, then by index
	std::vector<uint32_t> levelFirst;             // level d = levelNodes[levelFirst[d] .. levelFirst[d + 1])
	std::vector<RelinkRun> runs;

	uint32_t numLevels() const { return levelFirst.empty() ? 0u : (uint32_t) levelFirst.size() - 1u; }
	size_t permEntries() const { return (size_t) V * ( N - 1 ); }
	size_t nextEntries() const { return (size_t) K * N; }
	size_t posEntries() const { return (size_t) streams * N; }
	// device bytes of the static and the working tables
	size_t bytes() const {
		return sizeof( uint32_t ) * ( rankOf.size() + coldBefore.size() + childBase.size() + levelNodes.size() + levelFirst.size() )
		       + N + sizeof( uint32_t ) * ( permEntries() + nextEntries() + posEntries() );
	}
};

// The tables of a layout (1 - 3) for a nested tree (plan: refitNesting's parent and end) and its ranking.  The sizes follow
// packWalk's; the 31-bit record references are checked here, once.
inline int relinkTables( const SceneTree& tree, const RefitPlan& plan, uint32_t layout, RelinkTables* t, std::string* why ) {
	const uint32_t N = tree.size();

	if( layout < 1 || layout > 3 ) {
		return packFail( why, PBR_EINVAL, "re-link: layout %u is not a ray-ordered walk's", layout );
	}
	if( !plan.nested || plan.parent.size() != N || plan.end.size() != N ) {
		return packFail( why, PBR_ESTATE, "re-link: the tree is not properly nested (%s)", plan.why.c_str() );
	}

	t->layout = layout;
	t->N = N;
	t->compact = ( layout == PBR_WALK_EIGHT_ORDERS_COMPACT ) ? 1u : 0u;
	t->scheme = t->compact ? 2u : layout;
	t->K = ( t->scheme == 1 ) ? 6u : 8u;
	t->V = ( t->scheme == 1 ) ? 6u : 2u;
	t->streams = t->compact ? 1u : t->K;
	t->recordBytes = t->compact ? 64 : 32;

	if( (size_t) t->streams * N * t->recordBytes >= kRefLimit ) {
		return packFail( why, PBR_EINVAL, "re-link: %u streams of %u records exceed 2 GiB (record references are 31-bit byte offsets)", t->streams, N );
	}

	t->hotPerStream = (uint32_t) std::min<size_t>( tree.ranked.size(), kLdsStageBytes / ( t->recordBytes * (size_t) t->streams ) );
	t->hotSlots = t->hotPerStream * t->streams * (uint32_t) ( t->recordBytes / 32 );
	t->storageQuads = 2 + ( (size_t) t->streams * ( N - 1 ) + 1 ) * ( t->recordBytes / sizeof( Quad ) );

	t->rankOf.assign( N, kRelinkCold );

	for( uint32_t r = 0; r < t->hotPerStream; r++ ) {
		t->rankOf[tree.ranked[r]] = r;
	}

	t->coldBefore.assign( (size_t) N + 1, 0 );

	for( uint32_t n = 1; n < N; n++ ) {
		t->coldBefore[n + 1] = t->coldBefore[n] + ( ( t->rankOf[n] == kRelinkCold ) ? 1u : 0u );
	}

	// child lists: in container order; depth: parents come first
	t->childBase.assign( N, 0 );
	std::vector<uint32_t> depth( N, 0 ), perLevel;
	uint32_t children = 0;

	for( uint32_t i = 0; i < N; i++ ) {
		if( i > 0 ) {
			depth[i] = depth[plan.parent[i]] + 1;
		}
		if( tree.face0s[i] >= 0 ) {
			continue;
		}

		t->childBase[i] = children;

		for( uint32_t c = i + 1; c < plan.end[i]; c = plan.end[c] ) {
			children++;
		}

		if( depth[i] >= perLevel.size() ) {
			perLevel.resize( (size_t) depth[i] + 1, 0 );
		}

		perLevel[depth[i]]++;
	}

	if( children != N - 1 ) {
		return packFail( why, PBR_ESTATE, "re-link: the containers have %u children, the tree %u nodes below node 0", children, N - 1 );
	}

	t->levelFirst.assign( perLevel.size() + 1, 0 );

	for( size_t d = 0; d < perLevel.size(); d++ ) {
		t->levelFirst[d + 1] = t->levelFirst[d] + perLevel[d];
	}

	t->levelNodes.assign( t->levelFirst.back(), 0 );
	std::vector<uint32_t> fill( t->levelFirst.begin(), t->levelFirst.end() - 1 );

	for( uint32_t i = 0; i < N; i++ ) {
		if( tree.face0s[i] < 0 ) {
			t->levelNodes[fill[depth[i]]++] = i;
		}
	}

	t->runs.clear();

	for( uint32_t d = 0; d < t->numLevels(); d++ ) {
		const size_t items = (size_t) perLevel[d] * t->K;

		if( items <= kRelinkNarrow ) {
			if( !t->runs.empty() && t->runs.back().blocks == 1 && t->runs.back().threads == kRelinkNarrowThreads ) {
				t->runs.back().numLevels++;
			}
			else {
				t->runs.push_back( RelinkRun { d, 1, 1, kRelinkNarrowThreads } );
			}
		}
		else {
			t->runs.push_back( RelinkRun { d, 1, (uint32_t) ( ( items + kRelinkWideThreads - 1 ) / kRelinkWideThreads ), kRelinkWideThreads } );
		}
	}

	return PBR_OK;
}

// The re-link in plain C++: the layout's records from `boxes` (the tree's N nodes with the refitted boxes), through the
// steps above in the launches' order.  out->recordOf as packWalk gives it.
inline int relinkWalk( const SceneTree& tree, const RefitPlan& plan, uint32_t layout, const pbr_bvh_node* boxes, PackedWalk* out, std::string* why ) {
	RelinkTables t;
	const int status = relinkTables( tree, plan, layout, &t, why );

	if( status != PBR_OK ) {
		return status;
	}

	const uint32_t N = t.N;
	// the reference-order stream as the refit leaves it (storeBox, pt_refit.hpp): the steps read the boxes from there
	std::vector<RelinkQuad> refNodes( (size_t) N * 2, RelinkQuad { 0.0f, 0.0f, 0.0f, 0.0f } );

	for( uint32_t n = 1; n < N; n++ ) {
		RelinkQuad* rec = refNodes.data() + (size_t) plan.recordOf[n] * 2;
		rec[0] = RelinkQuad { boxes[n].bbMin.x, boxes[n].bbMin.y, boxes[n].bbMax.x, boxes[n].bbMax.y };
		rec[1] = RelinkQuad { boxes[n].bbMin.z, boxes[n].bbMax.z, 0.0f, 0.0f };
	}

	std::vector<unsigned char> axis( N, 0 );
	std::vector<uint32_t> perm( t.permEntries(), 0 ), pos( t.posEntries(), 0 );
	std::vector<int> next( t.nextEntries(), -1 );
	std::vector<RelinkQuad> storage( t.storageQuads, RelinkQuad { 0.0f, 0.0f, 0.0f, 0.0f } );
	int header[8] = {};

	RelinkView v;
	v.N = N;
	v.scheme = t.scheme;
	v.compact = t.compact;
	v.K = t.K;
	v.V = t.V;
	v.streams = t.streams;
	v.hotPerStream = t.hotPerStream;
	v.refNodes = refNodes.data();
	v.refRecordOf = plan.recordOf.data();
	v.info = plan.info.data();
	v.rankOf = t.rankOf.data();
	v.coldBefore = t.coldBefore.data();
	v.childBase = t.childBase.data();
	v.axis = axis.data();
	v.perm = perm.data();
	v.next = next.data();
	v.pos = pos.data();
	v.header = header;
	v.records = storage.data() + 2;

	for( uint32_t i : t.levelNodes ) {
		relinkSort( v, i );
	}

	uint32_t level = 0;

	for( const RelinkRun& run : t.runs ) {
		if( run.firstLevel != level ) {
			return packFail( why, PBR_ESTATE, "re-link: the launches skip level %u", level );
		}

		for( ; level < run.firstLevel + run.numLevels; level++ ) {
			for( uint32_t k = 0; k < t.K; k++ ) {
				for( uint32_t at = t.levelFirst[level]; at < t.levelFirst[level + 1]; at++ ) {
					relinkLevel( v, t.levelNodes[at], k );
				}
			}
		}
	}

	for( uint32_t k = 0; k < t.streams; k++ ) {
		for( uint32_t n = 1; n < N; n++ ) {
			if( t.compact ) {
				relinkRecordCompact( v, n );
			}
			else {
				relinkRecord32( v, n, k );
			}
		}
	}

	relinkHeader( v );
	std::memcpy( storage.data(), header, sizeof( header ) );
	std::memcpy( out->first, header, sizeof( out->first ) );
	out->storage.assign( t.storageQuads, Quad { 0.0f, 0.0f, 0.0f, 0.0f } );
	std::memcpy( out->storage.data(), storage.data(), sizeof( Quad ) * t.storageQuads );
	out->hotSlots = t.hotSlots;
	out->recordOf.assign( (size_t) t.streams * N, -1 );

	for( uint32_t k = 0; k < t.streams; k++ ) {
		for( uint32_t n = 1; n < N; n++ ) {
			out->recordOf[(size_t) k * N + n] = (int) relinkRecordOf( v, n, k );
		}
	}

	return PBR_OK;
}
