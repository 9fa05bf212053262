// pt_temporal.hpp — the temporal part of the variance-guided denoise (pbr_denoise_temporal; host side: pbr_hip.hip).
// Included by pbr_hip.hip only, behind pt_denoise_guided.hpp; exists once (no build flavour).
//
// pbr_denoise_guided filters {accumulated colour C, variance V of the pixel's mean} of ONE adaptive render.  `temporalIntegrate`
// puts the history of earlier calls in front of that filter — SVGF's temporal accumulation (Schied et al. 2017, section 4.1)
// for static geometry: the pixel's first hit is projected through the PREVIOUS call's camera, the previous integrated
// {colour, variance} is fetched there with the four bilinear taps that lie on the same surface, and blended with {C, V} by
// sample weight.  The result I is what the guided passes then filter, and — unfiltered — what the next call fetches.
//
// For the pixel (px, py), each operation in binary32 (the library is built -ffp-contract=off with correctly rounded
// divisions), dot( a, b ) = ( ax*bx + ay*by ) + az*bz; primes are the previous call's: eye', cu', cv', cw', halfPx' = pxDim' / 2,
// the buffers I', P', N', A' and the lengths L':
//   1. candidate   d = P.xyz - eye' for a hit pixel; for a miss pixel the CURRENT camera's cw + inner * halfPx as centreRay
//                  (pt_denoise.hpp) builds it before normalize (the sky is at infinity: the eyes' translation is ignored);
//                  a = dot( d, cu' ) / dot( cu', cu' ), b and c likewise with cv' and cw';  !( c > 0 ): no candidate;
//                  fx = ( a / ( c * halfPx' ) + (float) ( w - 1 ) ) * 0.5f, fy with b and h;  not finite: no candidate
//   2. taps        x0 = floorf( fx ), tx = fx - x0, y0 and ty likewise; taps ( x0 + i, y0 + j ), j outer, i inner, i, j in {0, 1},
//                  bw = ( i ? tx : 1 - tx ) * ( j ? ty : 1 - ty ).  Valid: inside the image, bw > 0, N'.w == N.w, I' finite in all
//                  four words, and for a hit centre A'.w == A.w, dot( N', N ) >= normal_cos and — unless sigma_world == 0 —
//                  squaredDistance3( P', P ) <= r * r, r = ( sigma_world * pxDim ) * P.w
//   3. history     S = sum bw over the valid taps in visiting order;  S > 0: Hc = sum bw * I'.rgb / S,
//                  Hv = sum ( bw * bw ) * I'.w / ( S * S ), Hl = L' of the valid tap with the largest bw (the first of equals)
//   4. blend       no history, C or V not finite, or max_history == 1: I = {C, V} bit for bit, L = 1;  else
//                  L = min( Hl + 1, max_history ), alpha = 1.0f / (float) L, I.rgb = Hc + alpha * ( C - Hc ),
//                  I.w = ( ( 1 - alpha ) * ( 1 - alpha ) ) * Hv + ( alpha * alpha ) * V
// This inverts centreRay for an orthogonal camera basis, which is what PathTracer::fillCameraBasis hands out (u = w x up,
// v = u x w, all normalized); for a basis that is not, the formula above is still what is computed.
//
// MOVING GEOMETRY (pbr_temporal_track_motion; host policy: pt_temporal_host.hpp).  When the vertices were updated since the
// history was made, `temporalMotion` runs in front: step 0 of the header's definition.  With V the current vertices, H those
// the history was made under, f the pixel's first-hit face (firstHitFeatures' faceOut), a, b, c = V[facesV[f].xyz] and
// a', b', c' the same corners from H:
//   0. motion      all nine coordinates equal: Pprev = P, nref = N bit for bit, len = 1, code 1.  Otherwise e1 = b - a,
//                  e2 = c - a, w = P.xyz - a;  d11 = dot( e1, e1 ), d12 = dot( e1, e2 ), d22 = dot( e2, e2 ), w1 = dot( w, e1 ),
//                  w2 = dot( w, e2 );  den = d11 * d22 - d12 * d12;  u = ( d22 * w1 - d12 * w2 ) / den,
//                  v = ( d11 * w2 - d12 * w1 ) / den;  e1' = b' - a', e2' = c' - a';  Pprev = ( a' + e1' * u ) + e2' * v;
//                  n = cross( e1, e2 ), n' = cross( e1', e2' ) (per component two products, one subtraction), n' = -n' if
//                  dot( N, n ) < 0;  nref = n' un-normalised, len = sqrtf( dot( n', n' ) );  code 2, or 3 if u, v or Pprev is
//                  not finite.  Planes: motion {Pprev, code}, reference {nref, len}; a miss pixel: zeros.
// temporalIntegrate< true > then reads the two planes for the hit pixels: step 1 starts from d = Pprev - eye' (code 3: no
// candidate), step 2 tests dot( N', nref ) >= normal_cos * len and squaredDistance3( P', Pprev ) <= r * r, r still from P.w.
// For an unmoved face these are the static tests to the bit ( normal_cos * 1.0f ), so one code path serves both.
// temporalMotion is a kernel of its own because its planes are an output (pbr_read_temporal_motion), and so that
// temporalIntegrate< false > stays the kernel it was.  Its gathers — facesV[f] and six vertices, 16 bytes each — are shared by
// the lanes that hit the same face, which is most of a wave on anything but the finest meshes.
//
// One thread per pixel, 64 x 4 blocks, no LDS.  Layout: the history is kept as the feature buffers are — four row-major W x H
// float4 planes {I', P', N', A'} and one of 32-bit lengths — so a tap is one aligned 16-byte load per plane, and under small
// motion a wave's 64 lanes x 4 taps fall into two neighbouring rows of each plane: lines that the neighbouring lanes and the
// block's other three rows fetch as well.  N' is read first (it decides hit / miss), I' last.  {C, V} arrives in the plane
// that I is written to (pixelVariance's `working`): every thread reads and writes its own pixel only.
#pragma once

#include "pt_denoise_guided.hpp"
#include "pt_denoise_host.hpp"   // TemporalArgs

namespace ptd {

__device__ __forceinline__ float dotPlain( f3 a, f3 b ) {
	return ( a.x * b.x + a.y * b.y ) + a.z * b.z;
}

__device__ __forceinline__ bool finite4( float4 v ) {
	return finite1( v.x ) && finite1( v.y ) && finite1( v.z ) && finite1( v.w );
}

__device__ __forceinline__ f3 crossPlain( f3 a, f3 b ) {
	return mk3( a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x );
}

// Step 0: where was the pixel's first hit when the history was made?  face: firstHitFeatures' faceOut; vertices / histVertices:
// V and H.  motion {Pprev, code} and reference {nref, len} out.
__global__ void temporalMotion( int width, int height, const int* face, const float4* position, const float4* normal,
                                const uint4* facesV, const float4* vertices, const float4* histVertices, float4* motion, float4* reference ) {
	const int x = (int) ( blockIdx.x * blockDim.x + threadIdx.x );
	const int y = (int) ( blockIdx.y * blockDim.y + threadIdx.y );

	if( x >= width || y >= height ) {
		return;
	}

	const size_t at = (size_t) y * (size_t) width + (size_t) x;
	const int f = face[at];

	if( f < 0 ) {
		motion[at] = make_float4( 0.0f, 0.0f, 0.0f, 0.0f );
		reference[at] = make_float4( 0.0f, 0.0f, 0.0f, 0.0f );
		return;
	}

	const uint4 fv = facesV[f];
	const float4 va = vertices[fv.x], vb = vertices[fv.y], vc = vertices[fv.z];
	const float4 ha = histVertices[fv.x], hb = histVertices[fv.y], hc = histVertices[fv.z];
	const float4 p0 = position[at], n0 = normal[at];
	const bool unmoved = va.x == ha.x && va.y == ha.y && va.z == ha.z && vb.x == hb.x && vb.y == hb.y && vb.z == hb.z
		&& vc.x == hc.x && vc.y == hc.y && vc.z == hc.z;

	if( unmoved ) {
		motion[at] = make_float4( p0.x, p0.y, p0.z, 1.0f );
		reference[at] = make_float4( n0.x, n0.y, n0.z, 1.0f );
		return;
	}

	const f3 a = mk3( va.x, va.y, va.z ), a2 = mk3( ha.x, ha.y, ha.z );
	const f3 e1 = mk3( vb.x, vb.y, vb.z ) - a, e2 = mk3( vc.x, vc.y, vc.z ) - a;
	const f3 w = mk3( p0.x, p0.y, p0.z ) - a;
	const float d11 = dotPlain( e1, e1 ), d12 = dotPlain( e1, e2 ), d22 = dotPlain( e2, e2 );
	const float w1 = dotPlain( w, e1 ), w2 = dotPlain( w, e2 );
	const float den = d11 * d22 - d12 * d12;
	const float u = ( d22 * w1 - d12 * w2 ) / den;
	const float v = ( d11 * w2 - d12 * w1 ) / den;
	const f3 e1p = mk3( hb.x, hb.y, hb.z ) - a2, e2p = mk3( hc.x, hc.y, hc.z ) - a2;
	const f3 pprev = ( a2 + e1p * u ) + e2p * v;
	const f3 n = crossPlain( e1, e2 );
	f3 n2 = crossPlain( e1p, e2p );

	if( dotPlain( mk3( n0.x, n0.y, n0.z ), n ) < 0.0f ) {
		n2 = mk3( -n2.x, -n2.y, -n2.z );
	}

	const float len = __builtin_sqrtf( dotPlain( n2, n2 ) );
	const bool finite = finite1( u ) && finite1( v ) && finite1( pprev.x ) && finite1( pprev.y ) && finite1( pprev.z );
	motion[at] = make_float4( pprev.x, pprev.y, pprev.z, finite ? 2.0f : 3.0f );
	reference[at] = make_float4( n2.x, n2.y, n2.z, len );
}

// working: {C, V} in, I out (in place).  prev*: the previous call's planes (not read without history).  lengths: L out.
// historyOut (may be null): {fx, fy, L, valid} per pixel.  MOTION: motion / reference are temporalMotion's planes, read for
// the hit pixels; < false > does not touch them (null) and is the kernel for static geometry, operation by operation.
template<bool MOTION>
__global__ void temporalIntegrate( const TemporalArgs A, float4* working, const float4* position, const float4* normal, const float4* albedo,
                                   const float4* prevI, const float4* prevPosition, const float4* prevNormal, const float4* prevAlbedo,
                                   const unsigned* prevLengths, unsigned* lengths, float4* historyOut,
                                   const float4* motion, const float4* reference ) {
	const int x = (int) ( blockIdx.x * blockDim.x + threadIdx.x );
	const int y = (int) ( blockIdx.y * blockDim.y + threadIdx.y );

	if( x >= A.width || y >= A.height ) {
		return;
	}

	const size_t at = (size_t) y * (size_t) A.width + (size_t) x;
	const float4 cv0 = working[at];
	const float none = __builtin_nanf( "" );
	float fx = none, fy = none;
	unsigned valid = 0, historyLength = 0;
	float sumR = 0.0f, sumG = 0.0f, sumB = 0.0f, sumV = 0.0f, sumW = 0.0f;

	if( A.hasHistory != 0 ) {
		const float4 p0 = position[at], n0 = normal[at], a0 = albedo[at];
		const bool hit = ( n0.w != 0.0f );
		// what the taps are tested against: the first hit itself, or — MOTION — where it was {Pprev, code} and the old face's
		// normal {nref, len}
		float4 pRef = p0, nRef = n0;
		float normalBound = A.normalCos;
		bool lost = false;

		if( MOTION && hit ) {
			pRef = motion[at];
			nRef = reference[at];
			normalBound = A.normalCos * nRef.w;
			lost = ( pRef.w == 3.0f );
		}

		// 1. the candidate
		f3 d;

		if( hit ) {
			d = mk3( pRef.x, pRef.y, pRef.z ) - ld3( A.eye );
		}
		else {
			const f3 cu = ld3( A.curCu );
			const f3 cv = ld3( A.curCv );
			f3 inner = ld3( A.curCamA );
			inner = inner + cu * ( 2.0f * (float) x );
			inner = inner + cv;
			inner = inner - ld3( A.curCvH );
			inner = inner + cv * ( 2.0f * (float) y );
			d = ld3( A.curCw ) + inner * A.curHalfPx;
		}

		const f3 pu = ld3( A.cu ), pv = ld3( A.cv ), pw = ld3( A.cw );
		const float a = dotPlain( d, pu ) / dotPlain( pu, pu );
		const float b = dotPlain( d, pv ) / dotPlain( pv, pv );
		const float c = dotPlain( d, pw ) / dotPlain( pw, pw );

		if( c > 0.0f && !lost ) {
			const float scale = c * A.halfPx;
			const float cx = ( a / scale + (float) ( A.width - 1 ) ) * 0.5f;
			const float cy = ( b / scale + (float) ( A.height - 1 ) ) * 0.5f;

			if( finite1( cx ) && finite1( cy ) ) {
				fx = cx;
				fy = cy;
			}
		}

		if( finite1( fx ) ) {
			// 2. the taps.  Inside the image is decided in float: a candidate far outside has no int to convert to
			const float x0 = floorf( fx ), y0 = floorf( fy );
			const float tx = fx - x0, ty = fy - y0;
			const float radius = A.worldScale * p0.w;
			const float radius2 = radius * radius;
			float best = 0.0f;

			for( int j = 0; j < 2; j++ ) {
				const float tyf = y0 + (float) j;

				if( !( tyf >= 0.0f && tyf <= (float) ( A.height - 1 ) ) ) {
					continue;
				}

				for( int i = 0; i < 2; i++ ) {
					const float txf = x0 + (float) i;

					if( !( txf >= 0.0f && txf <= (float) ( A.width - 1 ) ) ) {
						continue;
					}

					const float bw = ( i ? tx : 1.0f - tx ) * ( j ? ty : 1.0f - ty );

					if( !( bw > 0.0f ) ) {
						continue;
					}

					const size_t tap = (size_t) (int) tyf * (size_t) A.width + (size_t) (int) txf;
					const float4 n = prevNormal[tap];

					if( n.w != n0.w ) {
						continue;
					}

					if( hit ) {
						if( prevAlbedo[tap].w != a0.w ) {
							continue;
						}
						if( !( dotPlain( mk3( n.x, n.y, n.z ), mk3( nRef.x, nRef.y, nRef.z ) ) >= normalBound ) ) {
							continue;
						}
						if( A.worldTerm != 0 && !( squaredDistance3( prevPosition[tap], pRef ) <= radius2 ) ) {
							continue;
						}
					}

					const float4 h = prevI[tap];

					if( !finite4( h ) ) {
						continue;
					}

					valid |= 1u << ( j * 2 + i );
					sumR += bw * h.x;
					sumG += bw * h.y;
					sumB += bw * h.z;
					sumV += ( bw * bw ) * h.w;
					sumW += bw;

					if( bw > best ) {
						best = bw;
						historyLength = prevLengths[tap];
					}
				}
			}
		}
	}

	// 3. + 4. the history's value and the blend
	unsigned length = 1;
	float4 result = cv0;

	if( sumW > 0.0f && A.maxHistory > 1u && finite4( cv0 ) ) {
		const float hr = sumR / sumW, hg = sumG / sumW, hb = sumB / sumW;
		const float hv = sumV / ( sumW * sumW );
		length = ( historyLength + 1u < A.maxHistory ) ? historyLength + 1u : A.maxHistory;
		const float alpha = 1.0f / (float) length;
		const float keep = 1.0f - alpha;
		result.x = hr + alpha * ( cv0.x - hr );
		result.y = hg + alpha * ( cv0.y - hg );
		result.z = hb + alpha * ( cv0.z - hb );
		result.w = ( keep * keep ) * hv + ( alpha * alpha ) * cv0.w;
	}

	working[at] = result;
	lengths[at] = length;

	if( historyOut != nullptr ) {
		historyOut[at] = make_float4( fx, fy, (float) length, (float) valid );
	}
}

}  // namespace ptd
