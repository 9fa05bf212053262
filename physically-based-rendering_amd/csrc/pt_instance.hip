// One group of path-tracing kernels in one build flavour (pt_instances.hpp, pt_flavour.hpp):
//   hipcc -c -DPT_FLAVOUR=<0..3 | 5 | 7, + 8: chained> -DPT_GROUP=<0..9> pt_instance.hip
#if !defined( PT_FLAVOUR ) || !defined( PT_GROUP )
#error "pt_instance.hip is compiled once per (PT_FLAVOUR, PT_GROUP) pair: see build.py"
#endif

#include "pt_kernel.hpp"
#include "pt_instances.hpp"

#if PT_CHAINED && ( PT_GROUP == PTI_CHAIN || PT_GROUP == PTI_REFILL_PHONG || PT_GROUP == PTI_WALK )
#error "the chained flavours hold the seven plans' kernels only"
#endif

#if PT_GROUP == PTI_CHAIN
// the focus chain of this flavour: two kernels, with or without orb lights
#include "pt_chain.hpp"

extern "C" const void* PTI_NAME( PT_FLAVOUR, PT_GROUP )( uint32_t stage, int, int lights ) {
	if( stage == 0 ) {
		return lights ? (const void*) ptk::focusChainPixel<true> : (const void*) ptk::focusChainPixel<false>;
	}

	return lights ? (const void*) ptk::focusChainSlots<true> : (const void*) ptk::focusChainSlots<false>;
}
#elif PT_GROUP == PTI_WALK
// the per-ray entry into the walk of this flavour (pbr_diag_trace_walk): both walks, with and without the staged prefix,
// flat and Phong-tessellated faces, with or without orb lights
#include "pt_walk_diag.hpp"

namespace {

template<bool ANYHIT, bool USE_LDS>
const void* pickWalk( int phong, int lights ) {
	if( phong ) {
		return lights ? (const void*) ptk::diagTraceWalk<ANYHIT, true, USE_LDS, true> : (const void*) ptk::diagTraceWalk<ANYHIT, false, USE_LDS, true>;
	}

	return lights ? (const void*) ptk::diagTraceWalk<ANYHIT, true, USE_LDS, false> : (const void*) ptk::diagTraceWalk<ANYHIT, false, USE_LDS, false>;
}

}  // namespace

// ( walk, phong, lights ): walk bit 0 = the any-hit walk, bit 1 = through the staged prefix
extern "C" const void* PTI_NAME( PT_FLAVOUR, PT_GROUP )( uint32_t walk, int phong, int lights ) {
	switch( walk & 3u ) {
		case 0: return pickWalk<false, false>( phong, lights );
		case 1: return pickWalk<true, false>( phong, lights );
		case 2: return pickWalk<false, true>( phong, lights );
		default: return pickWalk<true, true>( phong, lights );
	}
}
#else

#if PT_GROUP == PTI_DUAL && PT_WALK_COMPACT == 1
#error "pathTracingDual has no node phase for the compact record: the compact flavours render plan 6 with the 6-waves state machine"
#endif
#if PT_GROUP == PTI_DUAL && !defined( PT_NODE_PHASE_ASM )
#error "pathTracingDual has no C++ node phase: PBR_GUARD builds render plan 6 with the 6-waves state machine"
#endif

namespace {

#if PT_GROUP == PTI_REFILL_LEAN
#define PTI_KERNEL( B, S, L ) ptk::pathTracing<B, S, L, 4, false>
#elif PT_GROUP == PTI_REFILL_MID
#define PTI_KERNEL( B, S, L ) ptk::pathTracing<B, S, L, 6, false>
#elif PT_GROUP == PTI_REFILL_WIDE
#define PTI_KERNEL( B, S, L ) ptk::pathTracing<B, S, L, 8, false>
#elif PT_GROUP == PTI_REFILL_PHONG
#define PTI_KERNEL( B, S, L ) ptk::pathTracing<B, S, L, 4, true>
#elif PT_GROUP == PTI_PHASED_LEAN
#define PTI_KERNEL( B, S, L ) ptk::pathTracingPhased<B, S, L, 4>
#elif PT_GROUP == PTI_PHASED_MID
#define PTI_KERNEL( B, S, L ) ptk::pathTracingPhased<B, S, L, 6>
#elif PT_GROUP == PTI_PHASED_WIDE
#define PTI_KERNEL( B, S, L ) ptk::pathTracingPhased<B, S, L, 8>
#elif PT_GROUP == PTI_DUAL
#define PTI_KERNEL( B, S, L ) ptk::pathTracingDual<B, S, L>
#else
#error "unknown PT_GROUP"
#endif

typedef void ( *Kernel )( const ptk::DevParams );

}  // namespace

extern "C" const void* PTI_NAME( PT_FLAVOUR, PT_GROUP )( uint32_t brdf, int shadow, int lights ) {
	Kernel k;

	if( brdf == 0 ) {
		k = lights ? ( shadow ? PTI_KERNEL( 0, true, true ) : PTI_KERNEL( 0, false, true ) ) : PTI_KERNEL( 0, false, false );
	}
	else {
		k = lights ? ( shadow ? PTI_KERNEL( 1, true, true ) : PTI_KERNEL( 1, false, true ) ) : PTI_KERNEL( 1, false, false );
	}

	return (const void*) k;
}

#endif   // PT_GROUP != PTI_CHAIN, PTI_WALK
