// pt_skin_host.hpp — pbr_set_skin / pbr_update_skin (include/pbr_hip.h): blend-weight skinning, computed on the device from a
// REST POSE.  One source for both sides, as pt_transform_host.hpp is: the kernels of pt_skin.hpp call blendMatrix, skinPosition
// and skinNormal on the device, pbr_hip.hip calls the argument checks and the repacking on the host, and tests/skin_driver.cpp
// (a plain C++17 compiler, -ffp-contract=off like the library) builds all of it without a device.  tests/skin_ref.py restates
// it in numpy.
//
// Operation by operation in binary32, none fused (the header has it in full).  An element — a vertex or a vertex normal — has
// four slots j = 0..3, each a bone index and a weight; a bone's matrix is row-major 3 x 4, pbr_update_transforms' layout.
//   slots      S = the slots whose weight compares unequal to 0, in slot order; a slot with weight 0 contributes nothing
//   blend      first slot s of S: B[k] = w_s * m_s[k]; every later one: B[k] = B[k] + w_s * m_s[k] (a product, then an addition)
//   position   p' = ptx::transformPosition( B, p ), its identity rule included
//   normal     ( c, det ) = ptx::cofactors( B ), n' = ptx::transformNormal( c, isIdentity( B ), n ): a d that is 0, infinite or
//              NaN copies the rest normal, so a singular blend is legal
// The weights are used as given: not normalised, their sum not checked.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "pt_transform_host.hpp"

namespace pts {

// An element's influences as they lie on the device: four bones, then four weights — 32 bytes, two quads.
struct Influence {
	uint32_t bones[PBR_SKIN_INFLUENCES];
	float weights[PBR_SKIN_INFLUENCES];
};

static_assert( sizeof( Influence ) == 32, "an influence record is two quads" );

// `records`: three quads per bone, the twelve words of its matrix (Q: float4 on the device, pbr_float4 on the host).  With no
// weight unequal to 0 — checkSkin refuses such an element — B is all zero.
template<class Q>
PATCH_FN void blendMatrix( const Q* records, const uint32_t bones[PBR_SKIN_INFLUENCES], const float weights[PBR_SKIN_INFLUENCES], float B[12] ) {
	bool first = true;

	for( int k = 0; k < 12; k++ ) {
		B[k] = 0.0f;
	}

	for( int j = 0; j < PBR_SKIN_INFLUENCES; j++ ) {
		const float w = weights[j];

		if( w != 0.0f ) {
			const Q* record = records + (size_t) bones[j] * 3;
			const Q r0 = record[0], r1 = record[1], r2 = record[2];
			const float m[12] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w };

			for( int k = 0; k < 12; k++ ) {
				const float term = w * m[k];
				B[k] = first ? term : B[k] + term;
			}

			first = false;
		}
	}
}

template<class Q, class P>
PATCH_FN P skinPosition( const Q* records, const uint32_t bones[PBR_SKIN_INFLUENCES], const float weights[PBR_SKIN_INFLUENCES], P p ) {
	float B[12];
	blendMatrix( records, bones, weights, B );
	return ptx::transformPosition( B, p );
}

template<class Q, class P>
PATCH_FN P skinNormal( const Q* records, const uint32_t bones[PBR_SKIN_INFLUENCES], const float weights[PBR_SKIN_INFLUENCES], P n ) {
	float B[12], c[9], det;
	blendMatrix( records, bones, weights, B );
	ptx::cofactors( B, c, &det );
	return ptx::transformNormal( c, ptx::isIdentity( B ), n );
}

}   // namespace pts

// ---- host only from here ----

// What pbr_set_skin answers to these arrays before it touches the device.  num_bones == 0 with all four pointers NULL drops
// the skin: PBR_OK.  `uploadedV` / `uploadedN` are the upload's counts.  The order is the header's.
inline int checkSkin( const uint32_t* vertex_bones, const float* vertex_weights, uint32_t num_vertices, uint32_t uploadedV, const uint32_t* normal_bones,
                      const float* normal_weights, uint32_t num_normals, uint32_t uploadedN, uint32_t num_bones, std::string* why ) {
	if( num_bones == 0 && vertex_bones == nullptr && vertex_weights == nullptr && normal_bones == nullptr && normal_weights == nullptr ) {
		return PBR_OK;
	}
	if( vertex_bones == nullptr || vertex_weights == nullptr ) {
		return packFail( why, PBR_EINVAL, "pbr_set_skin: null %s", ( vertex_bones == nullptr ) ? "vertex_bones" : "vertex_weights" );
	}
	if( num_vertices != uploadedV ) {
		return packFail( why, PBR_EINVAL, "pbr_set_skin: %u vertices, the uploaded scene has %u", num_vertices, uploadedV );
	}
	if( num_normals != 0 && num_normals != uploadedN ) {
		return packFail( why, PBR_EINVAL, "pbr_set_skin: %u normals, the uploaded scene has %u", num_normals, uploadedN );
	}
	if( ( normal_bones == nullptr ) != ( num_normals == 0 ) || ( normal_weights == nullptr ) != ( num_normals == 0 ) ) {
		return packFail( why, PBR_EINVAL, "pbr_set_skin: %s normal_bones and %s normal_weights with num_normals = %u (NULL, NULL and 0: the normals are never transformed)",
		                 ( normal_bones == nullptr ) ? "null" : "non-null", ( normal_weights == nullptr ) ? "null" : "non-null", num_normals );
	}
	if( num_bones == 0 ) {
		return packFail( why, PBR_EINVAL, "pbr_set_skin: num_bones = 0 with influences (0 bones and four NULL pointers drop the skin)" );
	}

	const uint32_t* bones[2] = { vertex_bones, normal_bones };
	const float* weights[2] = { vertex_weights, normal_weights };
	const uint32_t counts[2] = { num_vertices, num_normals };
	const char* names[2] = { "vertex", "normal" };

	for( int a = 0; a < 2; a++ ) {
		for( uint32_t i = 0; i < counts[a]; i++ ) {
			for( int j = 0; j < PBR_SKIN_INFLUENCES; j++ ) {
				if( bones[a][(size_t) i * PBR_SKIN_INFLUENCES + j] >= num_bones ) {
					return packFail( why, PBR_EINVAL, "pbr_set_skin: slot %d of %s %u names bone %u, there are %u bones", j, names[a], i,
					                 bones[a][(size_t) i * PBR_SKIN_INFLUENCES + j], num_bones );
				}
			}
		}
	}

	for( int a = 0; a < 2; a++ ) {
		for( uint32_t i = 0; i < counts[a]; i++ ) {
			for( int j = 0; j < PBR_SKIN_INFLUENCES; j++ ) {
				const float w = weights[a][(size_t) i * PBR_SKIN_INFLUENCES + j];

				if( !std::isfinite( w ) || w < 0.0f ) {
					return packFail( why, PBR_EINVAL, "pbr_set_skin: the weight in slot %d of %s %u is %g (it must be finite and not negative)", j, names[a], i, (double) w );
				}
			}
		}
	}

	for( int a = 0; a < 2; a++ ) {
		for( uint32_t i = 0; i < counts[a]; i++ ) {
			const float* w = weights[a] + (size_t) i * PBR_SKIN_INFLUENCES;

			if( w[0] == 0.0f && w[1] == 0.0f && w[2] == 0.0f && w[3] == 0.0f ) {
				return packFail( why, PBR_EINVAL, "pbr_set_skin: the four weights of %s %u are all 0", names[a], i );
			}
		}
	}

	return PBR_OK;
}

// The caller's two arrays as the one 32-byte record per element the kernels read.
inline void packInfluences( const uint32_t* bones, const float* weights, uint32_t count, pts::Influence* out ) {
	for( uint32_t i = 0; i < count; i++ ) {
		for( int j = 0; j < PBR_SKIN_INFLUENCES; j++ ) {
			out[i].bones[j] = bones[(size_t) i * PBR_SKIN_INFLUENCES + j];
			out[i].weights[j] = weights[(size_t) i * PBR_SKIN_INFLUENCES + j];
		}
	}
}

// What pbr_update_skin answers to these matrices before it touches the device, and the bone records that travel: `records`
// has room for three quads per bone (its content is undefined after a refusal).  `setBones` is pbr_set_skin's count, > 0.
// Bones are not checked for a zero determinant: the definition handles a singular blend.  `call` names the caller in the
// messages: pbr_update_pose (pt_morph_host.hpp) takes its matrices through here too.
inline int checkSkinMatrices( const float* matrices, uint32_t num_bones, uint32_t setBones, pbr_float4* records, std::string* why, const char* call = "pbr_update_skin" ) {
	if( matrices == nullptr ) {
		return packFail( why, PBR_EINVAL, "%s: null matrices", call );
	}
	if( num_bones != setBones ) {
		return packFail( why, PBR_EINVAL, "%s: %u matrices, pbr_set_skin declared %u bones", call, num_bones, setBones );
	}

	for( uint32_t k = 0; k < num_bones; k++ ) {
		for( int w = 0; w < 12; w++ ) {
			if( !std::isfinite( matrices[(size_t) k * 12 + w] ) ) {
				return packFail( why, PBR_EINVAL, "%s: word %d of bone %u's matrix is not finite", call, w, k );
			}
		}
	}

	for( size_t q = 0; q < (size_t) num_bones * 3; q++ ) {
		records[q] = { matrices[q * 4], matrices[q * 4 + 1], matrices[q * 4 + 2], matrices[q * 4 + 3] };
	}

	return PBR_OK;
}

// The skin of whole arrays in plain C++ (the device's result, word for word).  Returns the index of the first position that
// is not finite, or -1; the normal arguments may be null.
inline int64_t skinArrays( const pbr_float4* records, const pbr_float4* rest, const pts::Influence* vertex_influences, uint32_t num_vertices, pbr_float4* vertices_out,
                           const pbr_float4* rest_normals, const pts::Influence* normal_influences, uint32_t num_normals, pbr_float4* normals_out ) {
	int64_t bad = -1;

	for( uint32_t i = 0; i < num_vertices; i++ ) {
		vertices_out[i] = pts::skinPosition( records, vertex_influences[i].bones, vertex_influences[i].weights, rest[i] );

		if( bad < 0 && !ptx::finitePosition( vertices_out[i] ) ) {
			bad = i;
		}
	}

	for( uint32_t i = 0; rest_normals != nullptr && i < num_normals; i++ ) {
		normals_out[i] = pts::skinNormal( records, normal_influences[i].bones, normal_influences[i].weights, rest_normals[i] );
	}

	return bad;
}
