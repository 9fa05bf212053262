// Micro-benchmark (measurement aid, not product): what it costs a wave to reload a pointer from kernel-argument memory
// (s_load_dwordx2 through the scalar cache, always a hit after the first round) in front of a dependent global load, against
// holding the pointer in SGPRs across rounds — the shape of pathTracingDual's phase entries (csrc/pt_dual.hpp), where hipcc
// rematerialises DevParams members in front of a phase's first request.  A round is: [the reload], WORK independent vector
// instructions, s_waitcnt lgkmcnt(0), one dependent global_load_dword from a 16-KiB table (L1-resident), s_waitcnt vmcnt(0).
// WORK sweeps what stands between the load and its use; the difference RELOAD - PINNED per round is the exposed cost.
//   hipcc --offload-arch=gfx950 -O3 -o kernarg_reload kernarg_reload.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

#define TABLE_BYTES 16384u

template<bool RELOAD, int WORK>
__global__ __launch_bounds__( 1024 ) void rounds( const unsigned* table, int n, unsigned* out, long long* cycles ) {
	unsigned idx = ( threadIdx.x * 4u ) & ( TABLE_BYTES - 1u );   // byte offset into the table; the table holds byte offsets < TABLE_BYTES
	unsigned filler = threadIdx.x;
	const unsigned* pinned = table;
	asm volatile( "" : "+s"( pinned ) );      // opaque: not rematerialised from kernel-argument memory
	const auto kernarg = __builtin_amdgcn_kernarg_segment_ptr();   // `table` is at offset 0
	const long long t0 = clock64();

	for( int i = 0; i < n; i++ ) {
		if( RELOAD ) {
			const unsigned* p;
			asm volatile(
				"s_load_dwordx2 %[p], %[ka], 0x0\n"
				".rept %[work]\n"
				"v_add_u32 %[f], 1, %[f]\n"
				".endr\n"
				"s_waitcnt lgkmcnt(0)\n"
				"global_load_dword %[idx], %[idx], %[p]\n"
				"s_waitcnt vmcnt(0)\n"
				: [idx] "+v"( idx ), [f] "+v"( filler ), [p] "=&s"( p )
				: [ka] "s"( kernarg ), [work] "n"( WORK )
				: "memory"
			);
		}
		else {
			asm volatile(
				".rept %[work]\n"
				"v_add_u32 %[f], 1, %[f]\n"
				".endr\n"
				"s_waitcnt lgkmcnt(0)\n"
				"global_load_dword %[idx], %[idx], %[p]\n"
				"s_waitcnt vmcnt(0)\n"
				: [idx] "+v"( idx ), [f] "+v"( filler )
				: [p] "s"( pinned ), [work] "n"( WORK )
				: "memory"
			);
		}
	}

	const long long t1 = clock64();
	out[blockIdx.x * blockDim.x + threadIdx.x] = idx + filler;

	if( threadIdx.x == 0 && blockIdx.x == 0 ) {
		*cycles = t1 - t0;
	}
}

template<bool RELOAD, int WORK>
static void measure( const unsigned* table, unsigned* out, long long* cycles, int cus, int wavesPerSimd, int n, float* ms, long long* cyc ) {
	hipEvent_t e0, e1;
	(void) hipEventCreate( &e0 );
	(void) hipEventCreate( &e1 );
	const int threads = 256 * wavesPerSimd;    // 4 SIMDs x 64 lanes x waves per SIMD: one block per CU
	rounds<RELOAD, WORK><<<cus, threads>>>( table, 256, out, cycles );
	(void) hipEventRecord( e0 );
	rounds<RELOAD, WORK><<<cus, threads>>>( table, n, out, cycles );
	(void) hipEventRecord( e1 );
	(void) hipDeviceSynchronize();
	(void) hipEventElapsedTime( ms, e0, e1 );
	(void) hipMemcpy( cyc, cycles, sizeof( long long ), hipMemcpyDeviceToHost );
	(void) hipEventDestroy( e0 );
	(void) hipEventDestroy( e1 );
}

template<int WORK>
static void row( const unsigned* table, unsigned* out, long long* cycles, int cus, int n ) {
	for( int wps = 1; wps <= 4; wps *= 2 ) {
		float msP[3], msR[3];
		long long cyP[3], cyR[3];

		for( int rep = 0; rep < 3; rep++ ) {     // three alternating pairs, the minimum of each side
			measure<false, WORK>( table, out, cycles, cus, wps, n, &msP[rep], &cyP[rep] );
			measure<true, WORK>( table, out, cycles, cus, wps, n, &msR[rep], &cyR[rep] );
		}

		float bestP = msP[0], bestR = msR[0];
		long long cP = cyP[0], cR = cyR[0];

		for( int rep = 1; rep < 3; rep++ ) {
			if( msP[rep] < bestP ) { bestP = msP[rep]; }
			if( msR[rep] < bestR ) { bestR = msR[rep]; }
			if( cyP[rep] < cP ) { cP = cyP[rep]; }
			if( cyR[rep] < cR ) { cR = cyR[rep]; }
		}

		printf( "work %3d  waves/SIMD %d:  pinned %8.2f ns/round (%7.2f ticks)   reload %8.2f ns/round (%7.2f ticks)   reload - pinned %7.2f ns  %7.2f ticks of clock64\n",
			WORK, wps, bestP * 1e6 / n, (double) cP / n, bestR * 1e6 / n, (double) cR / n, ( bestR - bestP ) * 1e6 / n, (double) ( cR - cP ) / n );
	}
}

int main() {
	hipDeviceProp_t prop;

	if( hipGetDeviceProperties( &prop, 0 ) != hipSuccess ) {
		fprintf( stderr, "no HIP device\n" );
		return 1;
	}

	const int cus = prop.multiProcessorCount;
	printf( "%d CUs, clock %d kHz; a round = [s_load_dwordx2 of the table pointer], `work` x v_add_u32, s_waitcnt lgkmcnt(0), global_load_dword (16-KiB table), s_waitcnt vmcnt(0)\n", cus, prop.clockRate );
	std::vector<unsigned> host( TABLE_BYTES / 4 );

	for( unsigned i = 0; i < TABLE_BYTES / 4; i++ ) {
		host[i] = ( i * 4u + 4u * 67u ) & ( TABLE_BYTES - 1u );     // a chain of byte offsets, all inside the table
	}

	unsigned *table, *out;
	long long* cycles;
	(void) hipMalloc( &table, TABLE_BYTES );
	(void) hipMalloc( &out, sizeof( unsigned ) * cus * 1024 );
	(void) hipMalloc( &cycles, sizeof( long long ) );
	(void) hipMemcpy( table, host.data(), TABLE_BYTES, hipMemcpyHostToDevice );
	const int n = 100000;
	row<0>( table, out, cycles, cus, n );
	row<4>( table, out, cycles, cus, n );
	row<8>( table, out, cycles, cus, n );
	row<16>( table, out, cycles, cus, n );
	row<32>( table, out, cycles, cus, n );
	row<64>( table, out, cycles, cus, n );
	row<128>( table, out, cycles, cus, n );
	(void) hipFree( table );
	(void) hipFree( out );
	(void) hipFree( cycles );
	return 0;
}
