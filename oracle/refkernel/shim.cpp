/*
 * shim.cpp — the OpenCL builtins the reference's kernel text leaves undefined once a C compiler for the host has read it
 * (oracle/refkernel.py), and stand-ins for its three images.
 *
 * TEST INFRASTRUCTURE ONLY.  Own text: nothing here is taken from the reference.  Every arithmetic builtin follows the
 * table of oracle/pt_oracle.c ("Deterministic math layer"), operation for operation; the builtins whose bits are
 * implementation-defined or carry a ULP budget (sin, cos, tan, acos, atan, pow, cbrt) are not restated but CALLED in
 * liboracle.so through orc_math, so that there is one definition of them.  Build with -ffp-contract=off: a fused
 * multiply-add appears only where the table writes one.
 *
 * The names are the Itanium manglings clang gives the overloadable builtins of its OpenCL header; ext_vector_type vectors
 * mangle as OpenCL's do (Dv3_f ...).  The four names that hold OpenCL-only types get theirs through asm labels.
 * No <cmath>: it would declare pow, fabs, fmax ... itself.
 */
typedef float float3 __attribute__( ( ext_vector_type( 3 ) ) );
typedef float float4 __attribute__( ( ext_vector_type( 4 ) ) );
typedef int int2 __attribute__( ( ext_vector_type( 2 ) ) );

extern "C" void orc_math( int op, const float* x, const float* y, int n, float* out );

static inline float oracle_math( int op, float x, float y = 0.0f ) {
	float out;
	orc_math( op, &x, &y, 1, &out );
	return out;
}

/* ---- through orc_math: sin 0, cos 1, tan 2, acos 3, atan 4, pow 5, cbrt 7 */
float native_sin( float x ) { return oracle_math( 0, x ); }
float native_cos( float x ) { return oracle_math( 1, x ); }
float native_tan( float x ) { return oracle_math( 2, x ); }
float acos( float x ) { return oracle_math( 3, x ); }
float atan( float x ) { return oracle_math( 4, x ); }
float pow( float x, float y ) { return oracle_math( 5, x, y ); }
float cbrt( float x ) { return oracle_math( 7, x ); }

/* ---- written out as the table states them */
float native_recip( float x ) { return 1.0f / x; }
float3 native_recip( float3 v ) { return float3{ 1.0f / v.x, 1.0f / v.y, 1.0f / v.z }; }
float native_divide( float a, float b ) { return a / b; }
float native_sqrt( float x ) { return __builtin_sqrtf( x ); }

float dot( float3 a, float3 b ) {
	return __builtin_fmaf( a.z, b.z, __builtin_fmaf( a.y, b.y, a.x * b.x ) );
}

float3 cross( float3 a, float3 b ) {
	return float3{
		__builtin_fmaf( a.y, b.z, -( a.z * b.y ) ),
		__builtin_fmaf( a.z, b.x, -( a.x * b.z ) ),
		__builtin_fmaf( a.x, b.y, -( a.y * b.x ) )
	};
}

float3 fast_normalize( float3 v ) {
	const float inv = 1.0f / __builtin_sqrtf( dot( v, v ) );
	return float3{ v.x * inv, v.y * inv, v.z * inv };
}

float length( float3 v ) { return __builtin_sqrtf( dot( v, v ) ); }

float3 fma( float3 a, float3 b, float3 c ) {
	return float3{ __builtin_fmaf( a.x, b.x, c.x ), __builtin_fmaf( a.y, b.y, c.y ), __builtin_fmaf( a.z, b.z, c.z ) };
}

float fract( float x, float* whole ) __asm__( "_Z5fractfPU9CLprivatef" );
float fract( float x, float* whole ) {
	const float f = __builtin_floorf( x );
	*whole = f;
	return __builtin_fminf( x - f, 0x1.fffffep-1f );
}

float4 mix( float4 x, float4 y, float a ) {
	return float4{ x.x + ( y.x - x.x ) * a, x.y + ( y.y - x.y ) * a, x.z + ( y.z - x.z ) * a, x.w + ( y.w - x.w ) * a };
}

float fmin( float a, float b ) { return __builtin_fminf( a, b ); }
float fmax( float a, float b ) { return __builtin_fmaxf( a, b ); }
float3 fmin( float3 a, float3 b ) { return float3{ fmin( a.x, b.x ), fmin( a.y, b.y ), fmin( a.z, b.z ) }; }
float3 fmax( float3 a, float3 b ) { return float3{ fmax( a.x, b.x ), fmax( a.y, b.y ), fmax( a.z, b.z ) }; }
float fabs( float x ) { return __builtin_fabsf( x ); }
float3 fabs( float3 v ) { return float3{ fabs( v.x ), fabs( v.y ), fabs( v.z ) }; }
float max( float x, float y ) { return ( x < y ) ? y : x; }
float clamp( float x, float lo, float hi ) { return __builtin_fminf( __builtin_fmaxf( x, lo ), hi ); }
float4 clamp( float4 v, float lo, float hi ) {
	return float4{ clamp( v.x, lo, hi ), clamp( v.y, lo, hi ), clamp( v.z, lo, hi ), clamp( v.w, lo, hi ) };
}

/* ---- work-item id: one pixel at a time, set by the driver */
static thread_local unsigned long g_id[2];
extern "C" void rk_set_global_id( unsigned long x, unsigned long y ) { g_id[0] = x; g_id[1] = y; }
unsigned long get_global_id( unsigned int dim ) { return ( dim < 2 ) ? g_id[dim] : 0; }

/* ---- images: W x H float4, row-major; the only sampler the kernel makes is unnormalised, clamp-to-edge, nearest */
struct rk_image {
	float4* texels;
	int width, height;
};

extern "C" void* __translate_sampler_initializer( int ) { return nullptr; }

float4 rk_read_imagef( const rk_image* img, void* sampler, int2 pos ) __asm__( "_Z11read_imagef14ocl_image2d_ro11ocl_samplerDv2_i" );
float4 rk_read_imagef( const rk_image* img, void*, int2 pos ) {
	const int x = ( pos.x < 0 ) ? 0 : ( pos.x > img->width - 1 ) ? img->width - 1 : pos.x;
	const int y = ( pos.y < 0 ) ? 0 : ( pos.y > img->height - 1 ) ? img->height - 1 : pos.y;
	return img->texels[(long) y * img->width + x];
}

void rk_write_imagef( rk_image* img, int2 pos, float4 color ) __asm__( "_Z12write_imagef14ocl_image2d_woDv2_iDv4_f" );
void rk_write_imagef( rk_image* img, int2 pos, float4 color ) {
	if( pos.x >= 0 && pos.x < img->width && pos.y >= 0 && pos.y < img->height ) {
		img->texels[(long) pos.y * img->width + pos.x] = color;
	}
}

/*
 * Probe for tests/test_refkernel_cpu.py: the written-out builtins, callable from outside.  in: n x 12 floats, out: n x 4.
 *  0 native_recip(f)   1 native_recip(f3)   2 native_divide   3 native_sqrt   4 dot        5 cross   6 fast_normalize
 *  7 length            8 fma(f3)            9 fract {value, whole}            10 mix       11 fmin   12 fmax
 * 13 fmin(f3)         14 fmax(f3)          15 fabs           16 fabs(f3)     17 max       18 clamp  19 clamp(f4)
 * 20 native_sin       21 native_cos        22 native_tan     23 acos         24 atan      25 pow    26 cbrt
 * Operands are taken from in[0..] in order: vectors three (mix, clamp(f4): four) floats each, scalars one.
 */
extern "C" void rk_shim_probe( int op, const float* in, int n, float* out ) {
	for( int i = 0; i < n; i++ ) {
		const float* p = in + 12 * i;
		const float3 a = { p[0], p[1], p[2] }, b = { p[3], p[4], p[5] }, c = { p[6], p[7], p[8] };
		const float4 a4 = { p[0], p[1], p[2], p[3] }, b4 = { p[4], p[5], p[6], p[7] };
		float4 r = { 0.0f, 0.0f, 0.0f, 0.0f };
		float3 v = { 0.0f, 0.0f, 0.0f };
		float whole = 0.0f;
		switch( op ) {
			case 0: r.x = native_recip( p[0] ); break;
			case 1: v = native_recip( a ); break;
			case 2: r.x = native_divide( p[0], p[1] ); break;
			case 3: r.x = native_sqrt( p[0] ); break;
			case 4: r.x = dot( a, b ); break;
			case 5: v = cross( a, b ); break;
			case 6: v = fast_normalize( a ); break;
			case 7: r.x = length( a ); break;
			case 8: v = fma( a, b, c ); break;
			case 9: r.x = fract( p[0], &whole ); r.y = whole; break;
			case 10: r = mix( a4, b4, p[8] ); break;
			case 11: r.x = fmin( p[0], p[1] ); break;
			case 12: r.x = fmax( p[0], p[1] ); break;
			case 13: v = fmin( a, b ); break;
			case 14: v = fmax( a, b ); break;
			case 15: r.x = fabs( p[0] ); break;
			case 16: v = fabs( a ); break;
			case 17: r.x = max( p[0], p[1] ); break;
			case 18: r.x = clamp( p[0], p[1], p[2] ); break;
			case 19: r = clamp( a4, p[4], p[5] ); break;
			case 20: r.x = native_sin( p[0] ); break;
			case 21: r.x = native_cos( p[0] ); break;
			case 22: r.x = native_tan( p[0] ); break;
			case 23: r.x = acos( p[0] ); break;
			case 24: r.x = atan( p[0] ); break;
			case 25: r.x = pow( p[0], p[1] ); break;
			case 26: r.x = cbrt( p[0] ); break;
			default: break;
		}
		if( op == 1 || op == 5 || op == 6 || op == 8 || op == 13 || op == 14 || op == 16 ) {
			r = float4{ v.x, v.y, v.z, 0.0f };
		}
		out[4 * i + 0] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w;
	}
}
