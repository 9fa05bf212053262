// pt_morph_host.hpp — pbr_set_morph / pbr_update_morph / pbr_update_pose (include/pbr_hip.h): morph targets (blend shapes),
// computed on the device from a REST POSE, alone or in front of the skin.  One source for both sides, as pt_skin_host.hpp is: the
// kernels of pt_morph.hpp call morphPosition, morphNormal, posePosition and poseNormal on the device, pbr_hip.hip calls the
// argument checks and the repacking on the host, and tests/morph_driver.cpp (a plain C++17 compiler, -ffp-contract=off like the
// library) builds all of it without a device.  tests/morph_ref.py restates it in numpy.
//
// Operation by operation in binary32, none fused (the header has it in full).  An element — a vertex or a vertex normal — owns a
// RUN of entries, each a delta ( dx, dy, dz ) and the target it belongs to, in ascending target.
//   active     the entries whose target's weight compares unequal to 0; the others contribute nothing, not even a +0
//   position   p' = p; for every active entry in run order, per word c: p'.c = p'.c + w * d.c (a product, then an addition);
//              p'.w = p.w.  No active entry: the rest quad bit for bit
//   normal     q = n accumulated the same way; no active entry: n; else ptx::unitOrRest( q, n ) — transformNormal's tail: a
//              squared length that is 0, infinite or NaN copies the rest normal
//   pose       pts::skinPosition( B, p' ) and pts::skinNormal( B, n' ): the skin of the morphed rest pose
// The weights are used as given: negative ones and ones above 1 are legal.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "pt_skin_host.hpp"

namespace ptm {

// One delta as it lies on the device: 16 bytes, read with one load.
struct alignas( 16 ) Entry {
	float dx, dy, dz;
	uint32_t target;
};

static_assert( sizeof( Entry ) == 16, "a morph entry is one quad" );

// q = q + sum of w * d over the active entries first .. last-1, in that order.  Returns whether there was an active one.
PATCH_FN bool accumulate( const Entry* entries, uint32_t first, uint32_t last, const float* weights, ptp::V3& q ) {
	bool any = false;

	for( uint32_t e = first; e < last; e++ ) {
		const Entry d = entries[e];
		const float w = weights[d.target];

		if( w != 0.0f ) {
			q.x = q.x + w * d.dx;
			q.y = q.y + w * d.dy;
			q.z = q.z + w * d.dz;
			any = true;
		}
	}

	return any;
}

// Q: any quad of floats with x, y, z, w (float4 on the device, pbr_float4 on the host).
template<class Q>
PATCH_FN Q morphPosition( const Entry* entries, uint32_t first, uint32_t last, const float* weights, Q p ) {
	ptp::V3 q = { p.x, p.y, p.z };
	(void) accumulate( entries, first, last, weights, q );
	Q out = p;
	out.x = q.x;
	out.y = q.y;
	out.z = q.z;
	return out;
}

template<class Q>
PATCH_FN Q morphNormal( const Entry* entries, uint32_t first, uint32_t last, const float* weights, Q n ) {
	ptp::V3 q = { n.x, n.y, n.z };
	return accumulate( entries, first, last, weights, q ) ? ptx::unitOrRest( q, n ) : n;
}

// skin( morph( rest ) ): `records`, `bones` and `blend` are pts::skinPosition's arguments.
template<class R, class Q>
PATCH_FN Q posePosition( const Entry* entries, uint32_t first, uint32_t last, const float* weights, const R* records, const uint32_t bones[PBR_SKIN_INFLUENCES],
                         const float blend[PBR_SKIN_INFLUENCES], Q p ) {
	return pts::skinPosition( records, bones, blend, morphPosition( entries, first, last, weights, p ) );
}

template<class R, class Q>
PATCH_FN Q poseNormal( const Entry* entries, uint32_t first, uint32_t last, const float* weights, const R* records, const uint32_t bones[PBR_SKIN_INFLUENCES],
                       const float blend[PBR_SKIN_INFLUENCES], Q n ) {
	return pts::skinNormal( records, bones, blend, morphNormal( entries, first, last, weights, n ) );
}

}   // namespace ptm

// ---- host only from here ----

// What pbr_set_morph answers to these lists before it touches the device.  num_targets == 0 with all six pointers NULL drops the
// morph: PBR_OK.  `uploadedV` / `uploadedN` are the upload's counts.  The order is the header's; within one rule the vertex lists
// come before the normal lists.
inline int checkMorph( const uint32_t* vertex_first, const uint32_t* vertex_index, const pbr_float4* vertex_delta, const uint32_t* normal_first,
                       const uint32_t* normal_index, const pbr_float4* normal_delta, uint32_t num_targets, uint32_t uploadedV, uint32_t uploadedN, std::string* why ) {
	const bool anyPointer = ( vertex_first != nullptr || vertex_index != nullptr || vertex_delta != nullptr || normal_first != nullptr || normal_index != nullptr ||
	                          normal_delta != nullptr );

	if( num_targets == 0 ) {
		return anyPointer ? packFail( why, PBR_EINVAL, "pbr_set_morph: num_targets = 0 with target lists (0 targets and six NULL pointers drop the morph)" ) : PBR_OK;
	}
	if( vertex_first == nullptr || vertex_index == nullptr || vertex_delta == nullptr ) {
		return packFail( why, PBR_EINVAL, "pbr_set_morph: null %s", ( vertex_first == nullptr ) ? "vertex_first" : ( vertex_index == nullptr ) ? "vertex_index" : "vertex_delta" );
	}
	if( ( normal_first == nullptr ) != ( normal_index == nullptr ) || ( normal_first == nullptr ) != ( normal_delta == nullptr ) ) {
		return packFail( why, PBR_EINVAL, "pbr_set_morph: %s normal_first, %s normal_index and %s normal_delta (all three NULL: the normals are never morphed)",
		                 ( normal_first == nullptr ) ? "null" : "non-null", ( normal_index == nullptr ) ? "null" : "non-null", ( normal_delta == nullptr ) ? "null" : "non-null" );
	}

	const uint32_t* firsts[2] = { vertex_first, normal_first };
	const uint32_t* indices[2] = { vertex_index, normal_index };
	const pbr_float4* deltas[2] = { vertex_delta, normal_delta };
	const uint32_t counts[2] = { uploadedV, uploadedN };
	const char* names[2] = { "vertex", "normal" };
	const int lists = ( normal_first != nullptr ) ? 2 : 1;

	for( int a = 0; a < lists; a++ ) {
		if( firsts[a][0] != 0 ) {
			return packFail( why, PBR_EINVAL, "pbr_set_morph: %s_first[0] is %u, not 0", names[a], firsts[a][0] );
		}

		for( uint32_t t = 0; t < num_targets; t++ ) {
			if( firsts[a][t + 1] < firsts[a][t] ) {
				return packFail( why, PBR_EINVAL, "pbr_set_morph: %s_first decreases at target %u (%u after %u)", names[a], t, firsts[a][t + 1], firsts[a][t] );
			}
		}
	}

	for( int a = 0; a < lists; a++ ) {
		for( uint32_t t = 0; t < num_targets; t++ ) {
			for( uint32_t e = firsts[a][t]; e < firsts[a][t + 1]; e++ ) {
				if( indices[a][e] >= counts[a] ) {
					return packFail( why, PBR_EINVAL, "pbr_set_morph: entry %u of target %u names %s %u, the uploaded scene has %u", e - firsts[a][t], t, names[a],
					                 indices[a][e], counts[a] );
				}
			}
		}
	}

	for( int a = 0; a < lists; a++ ) {
		std::vector<uint32_t> seenBy( counts[a], 0u );   // target + 1 of the last target that named the element

		for( uint32_t t = 0; t < num_targets; t++ ) {
			for( uint32_t e = firsts[a][t]; e < firsts[a][t + 1]; e++ ) {
				if( seenBy[indices[a][e]] == t + 1 ) {
					return packFail( why, PBR_EINVAL, "pbr_set_morph: target %u names %s %u twice", t, names[a], indices[a][e] );
				}

				seenBy[indices[a][e]] = t + 1;
			}
		}
	}

	for( int a = 0; a < lists; a++ ) {
		for( uint32_t t = 0; t < num_targets; t++ ) {
			for( uint32_t e = firsts[a][t]; e < firsts[a][t + 1]; e++ ) {
				const pbr_float4 d = deltas[a][e];

				if( !std::isfinite( d.x ) || !std::isfinite( d.y ) || !std::isfinite( d.z ) ) {
					return packFail( why, PBR_EINVAL, "pbr_set_morph: the %s delta of entry %u of target %u is not finite", names[a], e - firsts[a][t], t );
				}
			}
		}
	}

	return PBR_OK;
}

// The caller's target-major lists as the element-major layout the kernels read: runFirst[count + 1] and one entry per delta,
// an element's run in ascending target — a stable counting sort over the elements.  The lists have passed checkMorph.
inline int packMorph( const uint32_t* first, const uint32_t* index, const pbr_float4* delta, uint32_t num_targets, uint32_t count, uint32_t* runFirst,
                      ptm::Entry* entries, std::string* why ) {
	const size_t total = first[num_targets];

	if( total > (size_t) UINT32_MAX ) {
		return packFail( why, PBR_EINVAL, "pbr_set_morph: %zu entries do not fit 32 bits", total );
	}

	for( uint32_t i = 0; i <= count; i++ ) {
		runFirst[i] = 0;
	}

	for( size_t e = 0; e < total; e++ ) {
		runFirst[index[e] + 1]++;
	}

	for( uint32_t i = 0; i < count; i++ ) {
		runFirst[i + 1] += runFirst[i];
	}

	std::vector<uint32_t> next( runFirst, runFirst + count );

	for( uint32_t t = 0; t < num_targets; t++ ) {
		for( uint32_t e = first[t]; e < first[t + 1]; e++ ) {
			entries[next[index[e]]++] = { delta[e].x, delta[e].y, delta[e].z, t };
		}
	}

	return PBR_OK;
}

// What pbr_update_morph and pbr_update_pose answer to these weights before they touch the device, and the table that travels:
// `table` has room for setTargets floats (its content is undefined after a refusal).  `setTargets` is pbr_set_morph's count, > 0.
inline int checkMorphWeights( const float* weights, uint32_t num_targets, uint32_t setTargets, float* table, std::string* why, const char* call ) {
	if( weights == nullptr ) {
		return packFail( why, PBR_EINVAL, "%s: null weights", call );
	}
	if( num_targets != setTargets ) {
		return packFail( why, PBR_EINVAL, "%s: %u weights, pbr_set_morph declared %u targets", call, num_targets, setTargets );
	}

	for( uint32_t t = 0; t < num_targets; t++ ) {
		if( !std::isfinite( weights[t] ) ) {
			return packFail( why, PBR_EINVAL, "%s: the weight of target %u is not finite", call, t );
		}
	}

	for( uint32_t t = 0; t < num_targets; t++ ) {
		table[t] = weights[t];
	}

	return PBR_OK;
}

// The morph of whole arrays in plain C++ (the device's result, word for word).  Returns the index of the first position that
// is not finite, or -1; the normal arguments may be null.
inline int64_t morphArrays( const float* weights, const pbr_float4* rest, const uint32_t* vertex_run, const ptm::Entry* vertex_entries, uint32_t num_vertices,
                            pbr_float4* vertices_out, const pbr_float4* rest_normals, const uint32_t* normal_run, const ptm::Entry* normal_entries, uint32_t num_normals,
                            pbr_float4* normals_out ) {
	int64_t bad = -1;

	for( uint32_t i = 0; i < num_vertices; i++ ) {
		vertices_out[i] = ptm::morphPosition( vertex_entries, vertex_run[i], vertex_run[i + 1], weights, rest[i] );

		if( bad < 0 && !ptx::finitePosition( vertices_out[i] ) ) {
			bad = i;
		}
	}

	for( uint32_t i = 0; normal_run != nullptr && i < num_normals; i++ ) {
		normals_out[i] = ptm::morphNormal( normal_entries, normal_run[i], normal_run[i + 1], weights, rest_normals[i] );
	}

	return bad;
}

// The pose of whole arrays: the skin of the morphed rest pose.  normal_run == nullptr: the normals are skinned unmorphed;
// normal_influences == nullptr: they are morphed and not skinned; both null: they are not written.
inline int64_t poseArrays( const float* weights, const pbr_float4* records, const pbr_float4* rest, const uint32_t* vertex_run, const ptm::Entry* vertex_entries,
                           const pts::Influence* vertex_influences, uint32_t num_vertices, pbr_float4* vertices_out, const pbr_float4* rest_normals,
                           const uint32_t* normal_run, const ptm::Entry* normal_entries, const pts::Influence* normal_influences, uint32_t num_normals,
                           pbr_float4* normals_out ) {
	int64_t bad = -1;

	for( uint32_t i = 0; i < num_vertices; i++ ) {
		vertices_out[i] = ptm::posePosition( vertex_entries, vertex_run[i], vertex_run[i + 1], weights, records, vertex_influences[i].bones, vertex_influences[i].weights, rest[i] );

		if( bad < 0 && !ptx::finitePosition( vertices_out[i] ) ) {
			bad = i;
		}
	}

	for( uint32_t i = 0; i < num_normals; i++ ) {
		if( normal_run != nullptr && normal_influences != nullptr ) {
			normals_out[i] = ptm::poseNormal( normal_entries, normal_run[i], normal_run[i + 1], weights, records, normal_influences[i].bones, normal_influences[i].weights, rest_normals[i] );
		}
		else if( normal_influences != nullptr ) {
			normals_out[i] = pts::skinNormal( records, normal_influences[i].bones, normal_influences[i].weights, rest_normals[i] );
		}
		else if( normal_run != nullptr ) {
			normals_out[i] = ptm::morphNormal( normal_entries, normal_run[i], normal_run[i + 1], weights, rest_normals[i] );
		}
	}

	return bad;
}
