// pt_transform_host.hpp — pbr_set_parts / pbr_update_transforms (include/pbr_hip.h): rigid or affine motion per PART of the
// scene, computed on the device from a REST POSE.  One source for both sides: the kernels of pt_transform.hpp call the
// per-vertex and per-normal functions below on the device, pbr_hip.hip calls the per-part step and the argument checks on the
// host, and tests/transform_driver.cpp (a plain C++17 compiler, -ffp-contract=off like the library) builds all of it without a
// device.  tests/transform_ref.py restates it in numpy.
//
// Operation by operation in binary32, none fused (the header has it in full).  Part k's matrix is row-major 3 x 4, rows
// r = 0, 1, 2 are m[4r .. 4r+3], a_r the first three words of row r, m[4r+3] the translation.
//   per part, on the host   c0 = cross( a1, a2 ), c1 = cross( a2, a0 ), c2 = cross( a0, a1 ), det = dot( a0, c0 );
//                           det < 0 negates every word of c0, c1, c2
//   position                p'.x = ( ( m0*p.x + m1*p.y ) + m2*p.z ) + m3, rows 1 and 2 likewise; p'.w = p.w
//   normal                  q.r = dot( c_r, n ); d = dot( q, q ); d > 0 and d < inf: n'.xyz = q * ( 1.0f / sqrtf( d ) ),
//                           else n'.xyz = n.xyz; n'.w = n.w
//   identity                a part whose twelve words compare equal, as floats, to the identity copies its rest words
// dot and cross are pt_patch_refit_host.hpp's.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "pt_patch_refit_host.hpp"

namespace ptx {

// A part as it travels: 24 words = 96 bytes.  The position kernel reads the first three quads, the normal kernel the last three.
struct PartRecord {
	float m[12];
	float c[9];
	uint32_t identity;   // 1: copy the rest words
	uint32_t pad[2];
};

static_assert( sizeof( PartRecord ) == 96, "a part record is six quads" );

PATCH_FN bool isIdentity( const float m[12] ) {
	bool same = true;

	for( int k = 0; k < 12; k++ ) {
		same = same && ( m[k] == ( ( k == 0 || k == 5 || k == 10 ) ? 1.0f : 0.0f ) );
	}

	return same;
}

PATCH_FN bool finiteWord( float v ) {
	return fabsf( v ) <= 3.40282346638528859812e+38f;   // false for NaN
}

// The per-part step.  *det is the determinant before the sign is taken out.
PATCH_FN void cofactors( const float m[12], float c[9], float* det ) {
	const ptp::V3 a0 = { m[0], m[1], m[2] }, a1 = { m[4], m[5], m[6] }, a2 = { m[8], m[9], m[10] };
	const ptp::V3 c0 = ptp::cross3( a1, a2 ), c1 = ptp::cross3( a2, a0 ), c2 = ptp::cross3( a0, a1 );
	*det = ptp::dot3( a0, c0 );
	const float rows[9] = { c0.x, c0.y, c0.z, c1.x, c1.y, c1.z, c2.x, c2.y, c2.z };

	for( int k = 0; k < 9; k++ ) {
		c[k] = ( *det < 0.0f ) ? -rows[k] : rows[k];
	}
}

// Q: any quad of floats with x, y, z, w (float4 on the device, pbr_float4 on the host).
template<class Q>
PATCH_FN Q transformPosition( const float m[12], Q p ) {
	if( isIdentity( m ) ) {
		return p;
	}

	Q out = p;
	out.x = ( ( m[0] * p.x + m[1] * p.y ) + m[2] * p.z ) + m[3];
	out.y = ( ( m[4] * p.x + m[5] * p.y ) + m[6] * p.z ) + m[7];
	out.z = ( ( m[8] * p.x + m[9] * p.y ) + m[10] * p.z ) + m[11];
	return out;
}

template<class Q>
PATCH_FN bool finitePosition( Q p ) {
	return finiteWord( p.x ) && finiteWord( p.y ) && finiteWord( p.z );
}

// The tail of every normal rule (transformNormal below, ptm::morphNormal in pt_morph_host.hpp): q to unit length with the rest
// quad's .w — or the rest normal, word for word, when q's squared length is 0, infinite or NaN.
template<class Q>
PATCH_FN Q unitOrRest( ptp::V3 q, Q n ) {
	const float d = ptp::dot3( q, q );

	if( !( d > 0.0f && d < INFINITY ) ) {
		return n;
	}

	const ptp::V3 unit = q * ( 1.0f / sqrtf( d ) );
	Q out = n;
	out.x = unit.x;
	out.y = unit.y;
	out.z = unit.z;
	return out;
}

template<class Q>
PATCH_FN Q transformNormal( const float c[9], bool identity, Q n ) {
	if( identity ) {
		return n;
	}

	const ptp::V3 v = { n.x, n.y, n.z };
	const ptp::V3 q = { ptp::dot3( { c[0], c[1], c[2] }, v ), ptp::dot3( { c[3], c[4], c[5] }, v ), ptp::dot3( { c[6], c[7], c[8] }, v ) };
	return unitOrRest( q, n );
}

}   // namespace ptx

// ---- host only from here ----

// What pbr_set_parts answers to these arrays before it touches the device.  num_parts == 0 with both pointers NULL (and both
// counts 0) drops the parts: PBR_OK.  `uploadedV` / `uploadedN` are the upload's counts.
inline int checkParts( const uint32_t* vertex_part, uint32_t num_vertices, uint32_t uploadedV, const uint32_t* normal_part, uint32_t num_normals,
                       uint32_t uploadedN, uint32_t num_parts, std::string* why ) {
	if( num_parts == 0 ) {
		if( vertex_part != nullptr || normal_part != nullptr ) {
			return packFail( why, PBR_EINVAL, "pbr_set_parts: num_parts = 0 with part indices (0 parts and two NULL pointers drop the parts)" );
		}

		return PBR_OK;
	}
	if( vertex_part == nullptr ) {
		return packFail( why, PBR_EINVAL, "pbr_set_parts: null vertex_part" );
	}
	if( num_vertices != uploadedV ) {
		return packFail( why, PBR_EINVAL, "pbr_set_parts: %u vertices, the uploaded scene has %u", num_vertices, uploadedV );
	}
	if( ( normal_part == nullptr ) != ( num_normals == 0 ) ) {
		return packFail( why, PBR_EINVAL, "pbr_set_parts: %s normal_part with num_normals = %u (NULL and 0: the normals are never transformed)", ( normal_part == nullptr ) ? "null" : "non-null", num_normals );
	}
	if( normal_part != nullptr && num_normals != uploadedN ) {
		return packFail( why, PBR_EINVAL, "pbr_set_parts: %u normals, the uploaded scene has %u", num_normals, uploadedN );
	}

	for( uint32_t i = 0; i < num_vertices; i++ ) {
		if( vertex_part[i] >= num_parts ) {
			return packFail( why, PBR_EINVAL, "pbr_set_parts: vertex %u is in part %u, there are %u parts", i, vertex_part[i], num_parts );
		}
	}

	for( uint32_t i = 0; i < num_normals; i++ ) {
		if( normal_part[i] >= num_parts ) {
			return packFail( why, PBR_EINVAL, "pbr_set_parts: normal %u is in part %u, there are %u parts", i, normal_part[i], num_parts );
		}
	}

	return PBR_OK;
}

// What pbr_update_transforms answers to these matrices before it touches the device, and the records that travel: `records`
// has room for num_parts of them (its content is undefined after a refusal).  `setParts` is pbr_set_parts' count, > 0.
inline int checkTransforms( const float* matrices, uint32_t num_parts, uint32_t setParts, ptx::PartRecord* records, std::string* why ) {
	if( matrices == nullptr ) {
		return packFail( why, PBR_EINVAL, "pbr_update_transforms: null matrices" );
	}
	if( num_parts != setParts ) {
		return packFail( why, PBR_EINVAL, "pbr_update_transforms: %u matrices, pbr_set_parts declared %u parts", num_parts, setParts );
	}

	for( uint32_t k = 0; k < num_parts; k++ ) {
		for( int w = 0; w < 12; w++ ) {
			if( !std::isfinite( matrices[(size_t) k * 12 + w] ) ) {
				return packFail( why, PBR_EINVAL, "pbr_update_transforms: word %d of part %u's matrix is not finite", w, k );
			}
		}
	}

	for( uint32_t k = 0; k < num_parts; k++ ) {
		ptx::PartRecord& r = records[k];
		float det = 0.0f;
		std::copy( matrices + (size_t) k * 12, matrices + (size_t) k * 12 + 12, r.m );
		ptx::cofactors( r.m, r.c, &det );
		r.identity = ptx::isIdentity( r.m ) ? 1u : 0u;
		r.pad[0] = r.pad[1] = 0u;

		if( !std::isfinite( det ) || det == 0.0f ) {
			return packFail( why, PBR_EINVAL, "pbr_update_transforms: part %u's matrix has determinant %g (it must be finite and not 0)", k, (double) det );
		}

		for( int w = 0; w < 9; w++ ) {
			if( !std::isfinite( r.c[w] ) ) {
				return packFail( why, PBR_EINVAL, "pbr_update_transforms: part %u's matrix has a cofactor that is not finite", k );
			}
		}
	}

	return PBR_OK;
}

// The transform of whole arrays in plain C++ (the device's result, word for word).  Returns the index of the first position
// that is not finite, or -1; normals may be null.
inline int64_t transformArrays( const ptx::PartRecord* records, const pbr_float4* rest, const uint32_t* vertex_part, uint32_t num_vertices, pbr_float4* vertices_out,
                                const pbr_float4* rest_normals, const uint32_t* normal_part, uint32_t num_normals, pbr_float4* normals_out ) {
	int64_t bad = -1;

	for( uint32_t i = 0; i < num_vertices; i++ ) {
		vertices_out[i] = ptx::transformPosition( records[vertex_part[i]].m, rest[i] );

		if( bad < 0 && !ptx::finitePosition( vertices_out[i] ) ) {
			bad = i;
		}
	}

	for( uint32_t i = 0; rest_normals != nullptr && i < num_normals; i++ ) {
		const ptx::PartRecord& r = records[normal_part[i]];
		normals_out[i] = ptx::transformNormal( r.c, r.identity != 0, rest_normals[i] );
	}

	return bad;
}
