// The stage diagnostics behind pbr_diag_math / pbr_diag_brdf / pbr_diag_new_ray / pbr_diag_solve_cubic /
// pbr_diag_phong_face / pbr_diag_camera_ray / pbr_diag_intersect / pbr_diag_surface_step (include/pbr_hip_diag.h): one thread per item.  Included by pt_aux.hpp (pbr_hip.hip: no flavour, the exact arithmetic) and by pt_diag_native.hip, which
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

// in: n x 8 {px, py, seed, tFocus, tObject, pad[3]}; out: n x 8 {origin, dir, seed after, 0} (as orc_camera_ray).  P carries
// the camera as a render call sets it (setCamera, pbr_hip.hip), the aperture and the configuration's anti-aliasing.
__global__ void diagCameraRay( const DevParams P, const float* in, int n, float* out ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( i >= n ) {
		return;
	}

	const float* p = in + (size_t) i * 8;
	float seed = p[2];
	const Ray ray = initRay( P, (int) p[0], (int) p[1], seed, p[3], p[4] );
	float* o = out + (size_t) i * 8;
	o[0] = ray.origin.x; o[1] = ray.origin.y; o[2] = ray.origin.z;
	o[3] = ray.dir.x; o[4] = ray.dir.y; o[5] = ray.dir.z;
	o[6] = seed;
	o[7] = 0.0f;
}

// in: n x 24, out: n x 4 (as orc_intersect).
// op 0 {A, B, C, origin, dir, rayT, tNear}: the face record as the upload and refitFaces form it, then triangleT -> {t, 0, 0, 0}
// op 1 {min, max, origin, dir, rayT}: the node record in boxHit's layout, the inverse direction as traverse forms it, then
//      boxHit<false> and boxHit<true> -> {closest-hit verdict, any-hit verdict, tNear, tFar}
// op 2 {pos, r, origin, dir}: intersectSphere -> {hit, tNear, 0, 0}
__global__ void diagIntersect( int op, const float* in, int n, float* out ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( i >= n ) {
		return;
	}

	const float* p = in + (size_t) i * 24;
	float* o = out + (size_t) i * 4;
	Ray ray;
	o[0] = o[1] = o[2] = o[3] = 0.0f;

	if( op == 0 ) {
		const f3 a = mk3( p[0], p[1], p[2] );
		const f3 b = mk3( p[3], p[4], p[5] );
		const f3 c = mk3( p[6], p[7], p[8] );
		const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
		const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
		TriRecord rec;
		rec.r0 = make_float4( a.x, a.y, a.z, e1x );
		rec.r1 = make_float4( e1y, e1z, e2x, e2y );
		rec.r2 = make_float4( e2z, 0.0f, 0.0f, 0.0f );
		ray.origin = mk3( p[9], p[10], p[11] );
		ray.dir = mk3( p[12], p[13], p[14] );
		o[0] = triangleT( rec, ray, p[15], p[16] );
	}
	else if( op == 1 ) {
		const float4 n0 = make_float4( p[0], p[1], p[3], p[4] );
		const float4 n1 = make_float4( p[2], p[5], 0.0f, 0.0f );
		ray.origin = mk3( p[6], p[7], p[8] );
		ray.dir = mk3( p[9], p[10], p[11] );
		const f3 invDir = mk3( div1( 1.0f, ray.dir.x ), div1( 1.0f, ray.dir.y ), div1( 1.0f, ray.dir.z ) );
		float tNear, tFar, tNearAny;
		const bool closest = boxHit<false>( n0, n1, ray, invDir, p[12], &tNear, &tFar );
		const bool any = boxHit<true>( n0, n1, ray, invDir, p[12], &tNearAny );
		o[0] = closest ? 1.0f : 0.0f;
		o[1] = any ? 1.0f : 0.0f;
		o[2] = tNear;
		o[3] = tFar;
	}
	else if( op == 2 ) {
		ray.origin = mk3( p[4], p[5], p[6] );
		ray.dir = mk3( p[7], p[8], p[9] );
		float tNear = 0.0f;
		const bool hit = intersectSphere( ray, mk3( p[0], p[1], p[2] ), p[3], &tNear );
		o[0] = hit ? 1.0f : 0.0f;
		o[1] = hit ? tNear : 0.0f;
	}
}

// The surface step of shadeStep (pt_kernel.hpp) from `seed += hit.t` to `color = color * throughput( ... )`, restated here
// statement by statement around the same device functions, with the template arguments of the lean lock-step kernel
// (pathTracing<.., 4>: CALLS = false, LATE = false): the new ray from the UNflipped normal, the flip, then the two
// evaluations with the tangent frame the new-ray stage left behind.  Material 0.
// in: n x 24 {origin, dir, normal, t, seed, color, lit, lightDir, lightRgb, pad[3]}; out: n x 12 {newDir, seed after, addDepth,
// color after, finalColor after (from 0), secondaryPaths increment} (as orc_surface_step)
template<int BRDF>
__global__ void diagSurfaceStep( const DevParams P, const float* in, int n, float* out ) {
	const int i = (int) ( blockIdx.x * blockDim.x + threadIdx.x );

	if( i >= n ) {
		return;
	}

	const float* p = in + (size_t) i * 24;
	const Material mtl = loadMaterial<false>( P, 0 );
	Ray ray;
	ray.origin = mk3( p[0], p[1], p[2] );
	ray.dir = mk3( p[3], p[4], p[5] );
	f3 normal = mk3( p[6], p[7], p[8] );
	const float t = p[9];
	float seed = p[10];
	f3 color = mk3( p[11], p[12], p[13] );
	const f3 lightDir = mk3( p[15], p[16], p[17] );
	const f3 lightRgb = mk3( p[18], p[19], p[20] );
	const bool lit = ( p[14] != 0.0f ) && ( lightRgb.x >= 0.0f );
	f3 finalColor = mk3( 0.0f, 0.0f, 0.0f );
	unsigned secondaryPaths = 0;
	bool addDepth = false;

	seed += t;

	TangentFrame frame;
	frame.valid = false;
	const f3 newDir = newRayDir<BRDF, false>( ray.dir, normal, mtl, seed, addDepth, &frame );

	if( dot( normal, -ray.dir ) <= 0.0f ) {
		normal = -normal;
	}

	if( lit ) {
		f3 add;

		if( shadowContribution<BRDF, false, false>( mtl, ray.dir, lightDir, normal, color, lightRgb, &add, &frame ) ) {
			finalColor = finalColor + add;
			secondaryPaths += 1;
		}
	}

	color = color * throughput<BRDF, false, false>( mtl, ray.dir, newDir, normal, &frame );

	float* o = out + (size_t) i * 12;
	o[0] = newDir.x; o[1] = newDir.y; o[2] = newDir.z;
	o[3] = seed;
	o[4] = addDepth ? 1.0f : 0.0f;
	o[5] = color.x; o[6] = color.y; o[7] = color.z;
	o[8] = finalColor.x; o[9] = finalColor.y; o[10] = finalColor.z;
	o[11] = (float) secondaryPaths;
}

}  // namespace ptk
