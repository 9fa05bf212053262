// Stand-in for <glm/glm.hpp>: the part of GLM the reference's host sources use (vec3 and eight functions), written for
// oracle/refhost.py.  TEST INFRASTRUCTURE ONLY — the product never includes it.
//
// GLM leaves no operation order open in what is used here, but it is not on the build machine, so the order is stated
// rather than inherited.  Every operation is one binary32 operation, none fused (the recipe compiles with
// -ffp-contract=off), componentwise unless said otherwise:
//   dot( a, b )     = ( a.x * b.x + a.y * b.y ) + a.z * b.z          (GLM's compute_dot<vec3>: tmp = a * b; tmp.x + tmp.y + tmp.z)
//   cross( a, b )   = ( a.y * b.z - b.y * a.z,  a.z * b.x - b.z * a.x,  a.x * b.y - b.x * a.y )
//   normalize( v )  = v * ( 1 / sqrt( dot( v, v ) ) )                (GLM: v * inversesqrt( dot( v, v ) ), inversesqrt = 1 / sqrt)
//   length( v )     = sqrt( dot( v, v ) )
//   min( x, y )     = ( y < x ) ? y : x                              (so min( x, NaN ) = x and min( NaN, y ) = NaN)
//   max( x, y )     = ( x < y ) ? y : x
//   abs( x )        = fabsf( x )
//   v * s, s * v    three multiplications;  v / s  three divisions;  a + b, a - b three additions / subtractions
// vec3() zero-initialises.  GLM leaves it uninitialised; the reference reads such a value in one place only, the right
// box of BVH::splitFaces (the mean split above bvh.sah_faces_limit), which none of the shipped models reaches.
// csrc/pt_patch_refit_host.hpp, host/bvh_builder.cpp and tests/patch_refit_ref.py take the same reading (parity).
#pragma once

#include <cmath>

namespace glm {

struct vec3 {
	float x, y, z;

	vec3() : x( 0.0f ), y( 0.0f ), z( 0.0f ) {}
	vec3( float x_, float y_, float z_ ) : x( x_ ), y( y_ ), z( z_ ) {}

	float& operator[]( int i ) { return ( i == 0 ) ? x : ( i == 1 ) ? y : z; }
	const float& operator[]( int i ) const { return ( i == 0 ) ? x : ( i == 1 ) ? y : z; }
};

inline vec3 operator+( const vec3& a, const vec3& b ) { return vec3( a.x + b.x, a.y + b.y, a.z + b.z ); }
inline vec3 operator-( const vec3& a, const vec3& b ) { return vec3( a.x - b.x, a.y - b.y, a.z - b.z ); }
inline vec3 operator*( const vec3& a, float s ) { return vec3( a.x * s, a.y * s, a.z * s ); }
inline vec3 operator*( float s, const vec3& a ) { return vec3( s * a.x, s * a.y, s * a.z ); }
inline vec3 operator/( const vec3& a, float s ) { return vec3( a.x / s, a.y / s, a.z / s ); }

inline float min( float x, float y ) { return ( y < x ) ? y : x; }
inline float max( float x, float y ) { return ( x < y ) ? y : x; }
inline float abs( float x ) { return std::fabs( x ); }

inline vec3 min( const vec3& a, const vec3& b ) { return vec3( min( a.x, b.x ), min( a.y, b.y ), min( a.z, b.z ) ); }
inline vec3 max( const vec3& a, const vec3& b ) { return vec3( max( a.x, b.x ), max( a.y, b.y ), max( a.z, b.z ) ); }

inline float dot( const vec3& a, const vec3& b ) { return ( a.x * b.x + a.y * b.y ) + a.z * b.z; }

inline vec3 cross( const vec3& a, const vec3& b ) {
	return vec3( a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y );
}

inline float length( const vec3& v ) { return std::sqrt( dot( v, v ) ); }
inline vec3 normalize( const vec3& v ) { return v * ( 1.0f / std::sqrt( dot( v, v ) ) ); }

}   // namespace glm
