// The stage diagnostics behind pbr_diag_math / pbr_diag_brdf / pbr_diag_new_ray / pbr_diag_solve_cubic /
// pbr_diag_phong_face (include/pbr_hip_diag.h): one thread per item.  Included by pt_aux.hpp (pbr_hip.hip: no flavour, the exact arithmetic) and by pt_diag_native.hip, which
// compiles them once more in the native-arithmetic flavour (PT_FLAVOUR=2, pt_flavour.hpp) for a context configured
// with pbr_config.arith = PBR_ARITH_NATIVE.
#pragma once

#include "pt_kernel.hpp"

namespace ptk {

__global__ void diagMath( int op, const float* x, const float* y, int n, float* out ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( i >= n ) {
		return;
	}

	float s, c;

	switch( op ) {
		case 0: sincos( x[i], &s, &c ); out[i] = s; break;
		case 1: sincos( x[i], &s, &c ); out[i] = c; break;
		case 2: out[i] = tan1( x[i] ); break;
		case 3: out[i] = acos1( x[i] ); break;
		case 4: out[i] = atan1( x[i] ); break;
		case 5: out[i] = pow1( x[i], y[i] ); break;
		case 6: out[i] = fract( sin1( x[i] ) * 43758.5453123f ); break;
		case 7: out[i] = cbrt1( x[i] ); break;
		default: out[i] = 0.0f; break;
	}
}

// in: n x 16 {out_dir, in_dir, normal, pad}; out: n x 4 (as orc_brdf_eval); material 0 of P.mats
template<int BRDF>
__global__ void diagBrdf( const DevParams P, const float* in, int n, float* out ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( i >= n ) {
		return;
	}

	const float* p = in + (size_t) i * 16;
	const Material mtl = loadMaterial( P, 0 );
	const f3 outDir = mk3( p[0], p[1], p[2] );
	const f3 inDir = mk3( p[3], p[4], p[5] );
	const f3 normal = mk3( p[6], p[7], p[8] );
	float* o = out + (size_t) i * 4;

	if( BRDF == 0 ) {
		float u, pdf;
		const float b = brdfSchlick( mtl, outDir, inDir, normal, &u, &pdf );
		o[0] = b; o[1] = u; o[2] = pdf; o[3] = 0.0f;
	}
	else {
		float spec, diff, dotHK1, pdf;
		brdfSA( mtl, outDir, inDir, normal, &spec, &diff, &dotHK1, &pdf );
		o[0] = spec; o[1] = diff; o[2] = dotHK1; o[3] = pdf;
	}
}

// in: n x 12 {origin, dir, normal, t, seed, pad}; out: n x 8 (as orc_new_ray); material 0
template<int BRDF>
__global__ void diagNewRay( const DevParams P, const float* in, int n, float* out ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( i >= n ) {
		return;
	}

	const float* p = in + (size_t) i * 12;
	const Material mtl = loadMaterial( P, 0 );
	const f3 origin = mk3( p[0], p[1], p[2] );
	const f3 dir = mk3( p[3], p[4], p[5] );
	const f3 normal = mk3( p[6], p[7], p[8] );
	float seed = p[10];
	bool addDepth = false;
	const f3 newOrigin = fma3( p[9], dir, origin );
	const f3 newDir = newRayDir<BRDF>( dir, normal, mtl, seed, addDepth );
	float* o = out + (size_t) i * 8;
	o[0] = newOrigin.x; o[1] = newOrigin.y; o[2] = newOrigin.z;
	o[3] = newDir.x; o[4] = newDir.y; o[5] = newDir.z;
	o[6] = seed;
	o[7] = addDepth ? 1.0f : 0.0f;
}

// in: n x 4 {a0, a1, a2, a3}; out: n x 4 {count, x0, x1, x2} (as orc_solve_cubic); the slots beyond count are 0
__global__ void diagSolveCubic( const float* in, int n, float* out ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( i >= n ) {
		return;
	}

	const float* p = in + (size_t) i * 4;
	float x[3] = { 0.0f, 0.0f, 0.0f };
	const int count = solveCubic( p[0], p[1], p[2], p[3], x );
	float* o = out + (size_t) i * 4;
	o[0] = (float) count;
	o[1] = ( count > 0 ) ? x[0] : 0.0f;
	o[2] = ( count > 1 ) ? x[1] : 0.0f;
	o[3] = ( count > 2 ) ? x[2] : 0.0f;
}

// in: n x 32 {P1, P2, P3, N1, N2, N3, origin, dir, rayT, tNear, tFar, alpha, pad[4]}; out: n x 4 {t, normal} (as
// orc_phong_face).  phongTessTriAndRayIntersect itself, not phongFaceT: equal normals are not diverted to the flat test.
__global__ void diagPhongFace( const float* in, int n, float* out ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( i >= n ) {
		return;
	}

	const float* p = in + (size_t) i * 32;
	Ray ray;
	ray.origin = mk3( p[18], p[19], p[20] );
	ray.dir = mk3( p[21], p[22], p[23] );
	f3 normal;
	const float t = phongTessTriAndRayIntersect(
		mk3( p[0], p[1], p[2] ), mk3( p[3], p[4], p[5] ), mk3( p[6], p[7], p[8] ),
		mk3( p[9], p[10], p[11] ), mk3( p[12], p[13], p[14] ), mk3( p[15], p[16], p[17] ),
		ray, p[24], p[25], p[26], p[27], &normal );
	float* o = out + (size_t) i * 4;
	o[0] = t; o[1] = normal.x; o[2] = normal.y; o[3] = normal.z;
}

}  // namespace ptk
