// pt_skin_dq_host.hpp — pbr_update_skin_dq / pbr_update_pose_dq / pbr_dual_quats_from_matrices (include/pbr_hip.h): dual-quaternion
// skinning over the influences and the rest pose pbr_set_skin captured.  One source for both sides, as pt_skin_host.hpp is: the
// kernels of pt_skin_dq.hpp call skinPositionDQ, skinNormalDQ, posePositionDQ and poseNormalDQ on the device, pbr_hip.hip calls the
// argument check and the conversion on the host, and tests/skin_dq_driver.cpp (a plain C++17 compiler, -ffp-contract=off like the
// library) builds all of it without a device.  tests/skin_dq_ref.py restates it in numpy.
//
// Operation by operation in binary32, none fused, sqrtf and `/` correctly rounded (the header has it in full).  A bone is eight
// words { rx, ry, rz, rw, dx, dy, dz, dw }: the rotation quaternion, vector part first, and the dual part 1/2 t r.
//   dot4        dot4( a, b ) = ( ( ax*bx + ay*by ) + az*bz ) + aw*bw
//   slots       S = the slots whose weight compares unequal to 0, in slot order (pbr_update_skin's rule)
//   hemisphere  the pivot is the real part of the first slot of S; a later slot s with dot4( r_s, pivot ) < 0 has its weight negated
//   blend       first slot: Q[k] = w * q_s[k]; later slots: Q[k] = Q[k] + w * q_s[k] (a product, then an addition), eight words
//   normalise   nn = dot4( Q.real, Q.real ), len = sqrtf( nn ), r = Q.real / len, d = Q.dual / len — a division per word
//   identity    r.x, r.y, r.z and the four words of d compare equal to 0 and fabsf( r.w ) == 1: the rest quad, bit for bit
//   position    t = 2.0f * cross( r.xyz, p ), u = cross( r.xyz, t ), p1 = ( p + r.w * t ) + u, c = cross( r.xyz, d.xyz ),
//               tr = 2.0f * ( ( r.w * d.xyz - d.w * r.xyz ) + c ), p' = p1 + tr, p'.w = p.w
//   normal      q = ( n + r.w * t ) + u with t and u from n, then ptx::unitOrRest( q, n ); !( nn > 0 && nn < inf ) copies the rest normal
// The bones are used as given: not checked for unit length (the blend is normalised), not checked for r . d = 0.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "pt_morph_host.hpp"

namespace ptq {

// An element's blend, normalised: r the rotation, d the dual part, nn the squared length the two were divided by the root of.
struct Blend {
	float r[4], d[4];
	float nn;
};

PATCH_FN float dot4( const float a[4], const float b[4] ) {
	return ( ( a[0] * b[0] + a[1] * b[1] ) + a[2] * b[2] ) + a[3] * b[3];
}

// `records`: two quads per bone, the real part and the dual part (Q: float4 on the device, pbr_float4 on the host).  With no
// weight unequal to 0 — checkSkin refuses such an element — every word of the blend is NaN.
template<class Q>
PATCH_FN Blend blendDualQuat( const Q* records, const uint32_t bones[PBR_SKIN_INFLUENCES], const float weights[PBR_SKIN_INFLUENCES] ) {
	float sum[8] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, pivot[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
	bool first = true;

	for( int j = 0; j < PBR_SKIN_INFLUENCES; j++ ) {
		float w = weights[j];

		if( w != 0.0f ) {
			const Q* record = records + (size_t) bones[j] * 2;
			const Q real = record[0], dual = record[1];
			const float q[8] = { real.x, real.y, real.z, real.w, dual.x, dual.y, dual.z, dual.w };

			if( first ) {
				for( int k = 0; k < 4; k++ ) {
					pivot[k] = q[k];
				}
			}
			else if( dot4( q, pivot ) < 0.0f ) {
				w = -w;
			}

			for( int k = 0; k < 8; k++ ) {
				const float term = w * q[k];
				sum[k] = first ? term : sum[k] + term;
			}

			first = false;
		}
	}

	Blend b;
	b.nn = dot4( sum, sum );
	const float len = sqrtf( b.nn );

	for( int k = 0; k < 4; k++ ) {
		b.r[k] = sum[k] / len;
		b.d[k] = sum[4 + k] / len;
	}

	return b;
}

PATCH_FN bool isIdentityDQ( const Blend& b ) {
	return b.r[0] == 0.0f && b.r[1] == 0.0f && b.r[2] == 0.0f && fabsf( b.r[3] ) == 1.0f && b.d[0] == 0.0f && b.d[1] == 0.0f && b.d[2] == 0.0f && b.d[3] == 0.0f;
}

// v turned by r: ( v + r.w * t ) + u, t = 2 cross( r.xyz, v ), u = cross( r.xyz, t )
PATCH_FN ptp::V3 rotateDQ( const Blend& b, ptp::V3 v ) {
	const ptp::V3 axis = { b.r[0], b.r[1], b.r[2] };
	const ptp::V3 t = 2.0f * ptp::cross3( axis, v );
	const ptp::V3 u = ptp::cross3( axis, t );
	return ( v + b.r[3] * t ) + u;
}

template<class P>
PATCH_FN P applyPositionDQ( const Blend& b, P p ) {
	if( isIdentityDQ( b ) ) {
		return p;
	}

	const ptp::V3 axis = { b.r[0], b.r[1], b.r[2] }, dual = { b.d[0], b.d[1], b.d[2] };
	const ptp::V3 turned = rotateDQ( b, { p.x, p.y, p.z } );
	const ptp::V3 c = ptp::cross3( axis, dual );
	const ptp::V3 tr = 2.0f * ( ( b.r[3] * dual - b.d[3] * axis ) + c );
	const ptp::V3 moved = turned + tr;
	P out = p;
	out.x = moved.x;
	out.y = moved.y;
	out.z = moved.z;
	return out;
}

template<class P>
PATCH_FN P applyNormalDQ( const Blend& b, P n ) {
	if( isIdentityDQ( b ) || !( b.nn > 0.0f && b.nn < INFINITY ) ) {
		return n;
	}

	return ptx::unitOrRest( rotateDQ( b, { n.x, n.y, n.z } ), n );
}

template<class Q, class P>
PATCH_FN P skinPositionDQ( const Q* records, const uint32_t bones[PBR_SKIN_INFLUENCES], const float weights[PBR_SKIN_INFLUENCES], P p ) {
	return applyPositionDQ( blendDualQuat( records, bones, weights ), p );
}

template<class Q, class P>
PATCH_FN P skinNormalDQ( const Q* records, const uint32_t bones[PBR_SKIN_INFLUENCES], const float weights[PBR_SKIN_INFLUENCES], P n ) {
	return applyNormalDQ( blendDualQuat( records, bones, weights ), n );
}

// dq skin( morph( rest ) ): the first four arguments are ptm::morphPosition's, the next three skinPositionDQ's.
template<class R, class Q>
PATCH_FN Q posePositionDQ( const ptm::Entry* entries, uint32_t first, uint32_t last, const float* weights, const R* records, const uint32_t bones[PBR_SKIN_INFLUENCES],
                           const float blend[PBR_SKIN_INFLUENCES], Q p ) {
	return skinPositionDQ( records, bones, blend, ptm::morphPosition( entries, first, last, weights, p ) );
}

template<class R, class Q>
PATCH_FN Q poseNormalDQ( const ptm::Entry* entries, uint32_t first, uint32_t last, const float* weights, const R* records, const uint32_t bones[PBR_SKIN_INFLUENCES],
                         const float blend[PBR_SKIN_INFLUENCES], Q n ) {
	return skinNormalDQ( records, bones, blend, ptm::morphNormal( entries, first, last, weights, n ) );
}

}   // namespace ptq

// ---- host only from here ----

// What pbr_update_skin_dq and pbr_update_pose_dq answer to these dual quaternions before they touch the device, and the bone
// records that travel: `records` has room for two quads per bone (its content is undefined after a refusal).  `setBones` is
// pbr_set_skin's count, > 0.  `call` names the caller in the messages.
inline int checkSkinDualQuats( const float* dual_quats, uint32_t num_bones, uint32_t setBones, pbr_float4* records, std::string* why, const char* call = "pbr_update_skin_dq" ) {
	if( dual_quats == nullptr ) {
		return packFail( why, PBR_EINVAL, "%s: null dual_quats", call );
	}
	if( num_bones != setBones ) {
		return packFail( why, PBR_EINVAL, "%s: %u dual quaternions, pbr_set_skin declared %u bones", call, num_bones, setBones );
	}

	for( uint32_t k = 0; k < num_bones; k++ ) {
		for( int w = 0; w < 8; w++ ) {
			if( !std::isfinite( dual_quats[(size_t) k * 8 + w] ) ) {
				return packFail( why, PBR_EINVAL, "%s: word %d of bone %u's dual quaternion is not finite", call, w, k );
			}
		}
	}

	for( uint32_t k = 0; k < num_bones; k++ ) {
		const float* q = dual_quats + (size_t) k * 8;

		if( q[0] == 0.0f && q[1] == 0.0f && q[2] == 0.0f && q[3] == 0.0f ) {
			return packFail( why, PBR_EINVAL, "%s: the real part of bone %u's dual quaternion is all 0 (it is the rotation: the identity is 0, 0, 0, 1)", call, k );
		}
	}

	for( size_t q = 0; q < (size_t) num_bones * 2; q++ ) {
		records[q] = { dual_quats[q * 4], dual_quats[q * 4 + 1], dual_quats[q * 4 + 2], dual_quats[q * 4 + 3] };
	}

	return PBR_OK;
}

// pbr_dual_quats_from_matrices: row-major 3 x 4 matrices, pbr_update_transforms' layout, to eight words per bone.  Computed in
// double, rounded once to float.  The 3 x 3 block must be a rotation: every word of R^T R - I and det - 1 within
// PBR_DQ_RIGID_TOLERANCE — an input rule, a dual quaternion carries neither scale nor shear nor a mirror.  `out` is not written
// for a refused call.
inline int dualQuatsFromMatrices( const float* matrices, uint32_t num_bones, float* out, std::string* why ) {
	const char* call = "pbr_dual_quats_from_matrices";

	if( matrices == nullptr || out == nullptr ) {
		return packFail( why, PBR_EINVAL, "%s: null %s", call, ( matrices == nullptr ) ? "matrices" : "dual_quats_out" );
	}

	for( uint32_t k = 0; k < num_bones; k++ ) {
		const float* m = matrices + (size_t) k * 12;

		for( int w = 0; w < 12; w++ ) {
			if( !std::isfinite( m[w] ) ) {
				return packFail( why, PBR_EINVAL, "%s: word %d of bone %u's matrix is not finite", call, w, k );
			}
		}

		const double R[3][3] = { { m[0], m[1], m[2] }, { m[4], m[5], m[6] }, { m[8], m[9], m[10] } };
		double worst = 0.0;

		for( int a = 0; a < 3; a++ ) {
			for( int b = 0; b < 3; b++ ) {
				const double gram = R[0][a] * R[0][b] + R[1][a] * R[1][b] + R[2][a] * R[2][b];
				worst = std::fmax( worst, std::fabs( gram - ( ( a == b ) ? 1.0 : 0.0 ) ) );
			}
		}

		const double det = R[0][0] * ( R[1][1] * R[2][2] - R[1][2] * R[2][1] ) - R[0][1] * ( R[1][0] * R[2][2] - R[1][2] * R[2][0] ) +
		                   R[0][2] * ( R[1][0] * R[2][1] - R[1][1] * R[2][0] );

		if( worst > PBR_DQ_RIGID_TOLERANCE || std::fabs( det - 1.0 ) > PBR_DQ_RIGID_TOLERANCE ) {
			return packFail( why, PBR_EINVAL, "%s: the 3 x 3 block of bone %u's matrix is not a rotation (|R^T R - I| = %g, det = %g, tolerance %g): a dual quaternion carries no scale, shear or mirror",
			                 call, k, worst, det, (double) PBR_DQ_RIGID_TOLERANCE );
		}
	}

	for( uint32_t k = 0; k < num_bones; k++ ) {
		const float* m = matrices + (size_t) k * 12;
		const double R[3][3] = { { m[0], m[1], m[2] }, { m[4], m[5], m[6] }, { m[8], m[9], m[10] } };
		const double t[3] = { m[3], m[7], m[11] };
		const double trace = R[0][0] + R[1][1] + R[2][2];
		double q[4];   // x, y, z, w

		// the largest of the four candidates under the root: no division by a small number, a half turn (w about 0) included
		if( trace > 0.0 ) {
			const double s = 2.0 * std::sqrt( 1.0 + trace );
			q[3] = 0.25 * s;
			q[0] = ( R[2][1] - R[1][2] ) / s;
			q[1] = ( R[0][2] - R[2][0] ) / s;
			q[2] = ( R[1][0] - R[0][1] ) / s;
		}
		else {
			const int i = ( R[0][0] >= R[1][1] && R[0][0] >= R[2][2] ) ? 0 : ( R[1][1] >= R[2][2] ) ? 1 : 2;
			const int j = ( i + 1 ) % 3, l = ( i + 2 ) % 3;
			const double s = 2.0 * std::sqrt( ( ( 1.0 + R[i][i] ) - R[j][j] ) - R[l][l] );
			q[i] = 0.25 * s;
			q[j] = ( R[j][i] + R[i][j] ) / s;
			q[l] = ( R[l][i] + R[i][l] ) / s;
			q[3] = ( R[l][j] - R[j][l] ) / s;
		}

		const double len = std::sqrt( ( q[0] * q[0] + q[1] * q[1] ) + ( q[2] * q[2] + q[3] * q[3] ) );

		for( int w = 0; w < 4; w++ ) {
			q[w] /= len;
		}

		// d = 1/2 ( t, 0 ) r; the last word as a difference from 0.0, so that the identity matrix gives +0 and not -0
		const double d[4] = { 0.5 * ( q[3] * t[0] + ( t[1] * q[2] - t[2] * q[1] ) ), 0.5 * ( q[3] * t[1] + ( t[2] * q[0] - t[0] * q[2] ) ),
		                      0.5 * ( q[3] * t[2] + ( t[0] * q[1] - t[1] * q[0] ) ), 0.0 - 0.5 * ( ( t[0] * q[0] + t[1] * q[1] ) + t[2] * q[2] ) };

		for( int w = 0; w < 4; w++ ) {
			out[(size_t) k * 8 + w] = (float) q[w];
			out[(size_t) k * 8 + 4 + w] = (float) d[w];
		}
	}

	return PBR_OK;
}

// The dq skin of whole arrays in plain C++ (the device's result, word for word).  Returns the index of the first position that
// is not finite, or -1; the normal arguments may be null.
inline int64_t skinArraysDQ( const pbr_float4* records, const pbr_float4* rest, const pts::Influence* vertex_influences, uint32_t num_vertices, pbr_float4* vertices_out,
                             const pbr_float4* rest_normals, const pts::Influence* normal_influences, uint32_t num_normals, pbr_float4* normals_out ) {
	int64_t bad = -1;

	for( uint32_t i = 0; i < num_vertices; i++ ) {
		vertices_out[i] = ptq::skinPositionDQ( records, vertex_influences[i].bones, vertex_influences[i].weights, rest[i] );

		if( bad < 0 && !ptx::finitePosition( vertices_out[i] ) ) {
			bad = i;
		}
	}

	for( uint32_t i = 0; rest_normals != nullptr && i < num_normals; i++ ) {
		normals_out[i] = ptq::skinNormalDQ( records, normal_influences[i].bones, normal_influences[i].weights, rest_normals[i] );
	}

	return bad;
}

// The dq pose of whole arrays: the dq skin of the morphed rest pose.  normal_run == nullptr: the normals are skinned unmorphed;
// normal_influences == nullptr: they are morphed and not skinned; both null: they are not written.
inline int64_t poseArraysDQ( const float* weights, const pbr_float4* records, const pbr_float4* rest, const uint32_t* vertex_run, const ptm::Entry* vertex_entries,
                             const pts::Influence* vertex_influences, uint32_t num_vertices, pbr_float4* vertices_out, const pbr_float4* rest_normals,
                             const uint32_t* normal_run, const ptm::Entry* normal_entries, const pts::Influence* normal_influences, uint32_t num_normals,
                             pbr_float4* normals_out ) {
	int64_t bad = -1;

	for( uint32_t i = 0; i < num_vertices; i++ ) {
		vertices_out[i] = ptq::posePositionDQ( vertex_entries, vertex_run[i], vertex_run[i + 1], weights, records, vertex_influences[i].bones, vertex_influences[i].weights, rest[i] );

		if( bad < 0 && !ptx::finitePosition( vertices_out[i] ) ) {
			bad = i;
		}
	}

	for( uint32_t i = 0; i < num_normals; i++ ) {
		if( normal_run != nullptr && normal_influences != nullptr ) {
			normals_out[i] = ptq::poseNormalDQ( normal_entries, normal_run[i], normal_run[i + 1], weights, records, normal_influences[i].bones, normal_influences[i].weights, rest_normals[i] );
		}
		else if( normal_influences != nullptr ) {
			normals_out[i] = ptq::skinNormalDQ( records, normal_influences[i].bones, normal_influences[i].weights, rest_normals[i] );
		}
		else if( normal_run != nullptr ) {
			normals_out[i] = ptm::morphNormal( normal_entries, normal_run[i], normal_run[i + 1], weights, rest_normals[i] );
		}
	}

	return bad;
}
