// csrc/pt_device_memory.hpp over malloc / free: the header's four primitives with a count of live allocations, a log of what
// was asked for and a switch that fails the k-th allocation, and a handful of buffers tests/test_device_memory_cpu.py moves
// through ctypes.  With -DDEVICE_MEMORY_DRIVER_MAIN a program of its own that runs the same moves (for the host sanitizers).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "pt_device_memory.hpp"

namespace {

enum { kDevice = 0, kPinned = 1 };
const int kFailure = 2;   // what hipErrorOutOfMemory is to the runtime

std::map<void*, int> gLive;           // pointer -> the space it came from
std::vector<uint64_t> gAsked;         // bytes of every allocation that was asked for, failed ones too
std::vector<char> gEvents;            // 'a' an allocation that succeeded, 'f' a release
int gFailAt = -1;                     // this many allocations from now, one fails (-1: none)
int gNullReleases = 0, gWrongSpace = 0;

int allocate( int space, void** p, size_t bytes ) {
	gAsked.push_back( bytes );

	if( gFailAt == 0 ) {
		gFailAt = -1;
		return kFailure;
	}

	gFailAt -= ( gFailAt > 0 ) ? 1 : 0;
	*p = std::malloc( bytes );
	gLive[*p] = space;
	gEvents.push_back( 'a' );
	return 0;
}

void release( int space, void* p ) {
	if( p == nullptr ) {
		gNullReleases++;
		return;
	}

	const auto at = gLive.find( p );

	if( at == gLive.end() || at->second != space ) {
		gWrongSpace++;
		return;
	}

	gLive.erase( at );
	gEvents.push_back( 'f' );
	std::free( p );
}

}  // namespace

namespace ptmem {

int deviceAlloc( void** p, size_t bytes ) { return allocate( kDevice, p, bytes ); }
void deviceFree( void* p ) { release( kDevice, p ); }
int pinnedAlloc( void** p, size_t bytes ) { return allocate( kPinned, p, bytes ); }
void pinnedFree( void* p ) { release( kPinned, p ); }

}  // namespace ptmem

namespace {

using ptmem::Owned;
using ptmem::Pinned;
using ptmem::allocAll;
using ptmem::want;

const int kSlots = 4;
Owned<float> gBuffers[kSlots];        // 4-byte elements: fewer than four of them are under the 16-byte floor

// a record shaped like pbr_hip.hip's PartsState: a nested pose, device and pinned members, plain values
struct Pose {
	Owned<float> rest, restNormals, staged;
	Owned<unsigned> flag;
	Owned<unsigned, Pinned> hostFlag;
	bool normals = false;
	uint64_t bytes = 0;
};

struct Parts {
	Pose pose;
	uint32_t count = 0;
	Owned<unsigned> ofVertex, ofNormal;
	Owned<double> records;
	Owned<double, Pinned> hostRecords;
};

int makeParts( Parts* out, uint32_t count, size_t vertices ) {
	Parts fresh;
	int err = allocAll( { want( fresh.pose.rest, vertices ), want( fresh.pose.staged, vertices ), want( fresh.pose.flag, 1 ), want( fresh.pose.hostFlag, 1 ) } );
	err = ( err != 0 ) ? err : allocAll( { want( fresh.ofVertex, vertices ), want( fresh.records, count ), want( fresh.hostRecords, count ) } );

	if( err != 0 ) {
		return err;       // fresh goes out of scope: nothing is kept
	}

	fresh.count = count;
	fresh.pose.bytes = 12 * vertices;
	*out = std::move( fresh );
	return 0;
}

// the five buffers of dm_alloc_all: two spaces, three element types
Owned<float> gA, gB;
Owned<unsigned char> gC;
Owned<double, Pinned> gD;
Owned<float, Pinned> gE;

}  // namespace

extern "C" {

void dm_reset( void ) {
	for( Owned<float>& b : gBuffers ) {
		b.reset();
	}

	gA.reset();
	gB.reset();
	gC.reset();
	gD.reset();
	gE.reset();
	gAsked.clear();
	gEvents.clear();
	gFailAt = -1;
	gNullReleases = gWrongSpace = 0;
}

int dm_live( void ) { return (int) gLive.size(); }
int dm_null_releases( void ) { return gNullReleases; }
int dm_wrong_space( void ) { return gWrongSpace; }
void dm_fail_at( int k ) { gFailAt = k; }

// the bytes asked for so far, and the successful allocations and releases as a string of 'a' and 'f'
int dm_asked( uint64_t* out, int capacity ) {
	for( int i = 0; i < (int) gAsked.size() && i < capacity; i++ ) {
		out[i] = gAsked[i];
	}

	return (int) gAsked.size();
}

int dm_events( char* out, int capacity ) {
	int n = 0;

	for( ; n < (int) gEvents.size() && n + 1 < capacity; n++ ) {
		out[n] = gEvents[n];
	}

	out[n] = 0;
	return (int) gEvents.size();
}

int dm_alloc( int slot, uint64_t count ) { return gBuffers[slot].alloc( (size_t) count ); }
int dm_grow( int slot, uint64_t count ) { return gBuffers[slot].grow( (size_t) count ); }
void dm_release( int slot ) { gBuffers[slot].reset(); }
void dm_swap( int a, int b ) { gBuffers[a].swap( gBuffers[b] ); }
void dm_move( int dst, int src ) { gBuffers[dst] = std::move( gBuffers[src] ); }

// {pointer, count, bytes, empty, the pointer the conversion gives}
void dm_state( int slot, uint64_t out[5] ) {
	const Owned<float>& b = gBuffers[slot];
	const float* converted = b;
	out[0] = (uint64_t) (uintptr_t) b.get();
	out[1] = b.count();
	out[2] = b.bytes();
	out[3] = b.empty() ? 1 : 0;
	out[4] = (uint64_t) (uintptr_t) converted;
}

// all or nothing over five buffers, the first of which holds something already; -> the status, emptied[i] = 1 for an empty one
int dm_alloc_all( uint64_t count, int emptied[5] ) {
	const int err = allocAll( { want( gA, (size_t) count ), want( gB, (size_t) count + 1 ), want( gC, (size_t) count + 2 ), want( gD, (size_t) count + 3 ), want( gE, 0 ) } );
	const bool empty[5] = { gA.empty(), gB.empty(), gC.empty(), gD.empty(), gE.empty() };

	for( int i = 0; i < 5; i++ ) {
		emptied[i] = empty[i] ? 1 : 0;
	}

	return err;
}

int dm_alloc_all_live( void ) {
	return ( gA.empty() ? 0 : 1 ) + ( gB.empty() ? 0 : 1 ) + ( gC.empty() ? 0 : 1 ) + ( gD.empty() ? 0 : 1 ) + ( gE.empty() ? 0 : 1 );
}

// A record like PartsState: built, moved into a holder that already owns one, replaced by an empty record.  out = the live
// allocations {with the first one held, with both built, after the move, after the empty record}, -> the holder's count in between
uint32_t dm_record( int out[4] ) {
	Parts holder;

	if( makeParts( &holder, 3, 10 ) != 0 ) {
		return 0;
	}

	out[0] = (int) gLive.size();
	Parts fresh;

	if( makeParts( &fresh, 5, 20 ) != 0 ) {
		return 0;
	}

	out[1] = (int) gLive.size();
	holder = std::move( fresh );
	out[2] = (int) gLive.size();
	const uint32_t count = holder.count + ( fresh.pose.rest.empty() && fresh.hostRecords.empty() ? 0 : 1000 );
	holder = Parts();
	out[3] = (int) gLive.size();
	return count;
}

// a record whose k-th allocation fails: -> the status, *live = what is held afterwards
int dm_record_fails( int k, int* live ) {
	int err = 0;
	{
		Parts parts;
		gFailAt = k;
		err = makeParts( &parts, 5, 20 );
		gFailAt = -1;
	}
	*live = (int) gLive.size();
	return err;
}

}  // extern "C"

#ifdef DEVICE_MEMORY_DRIVER_MAIN
#define CHECK( what ) \
	do { \
		if( !( what ) ) { \
			std::printf( "device memory driver: line %d: %s\n", __LINE__, #what ); \
			return 1; \
		} \
	} while( 0 )

int main() {
	uint64_t s[5], t[5];
	dm_reset();
	CHECK( dm_alloc( 0, 0 ) == 0 && dm_alloc( 1, 100 ) == 0 && dm_live() == 2 );
	dm_state( 0, s );
	CHECK( s[0] != 0 && s[1] == 0 && s[2] == 0 && s[3] == 0 && s[4] == s[0] );
	dm_move( 0, 1 );
	dm_state( 0, s );
	dm_state( 1, t );
	CHECK( dm_live() == 1 && s[1] == 100 && s[2] == 400 && t[0] == 0 && t[3] == 1 );
	dm_move( 0, 0 );
	CHECK( dm_live() == 1 );
	CHECK( dm_grow( 0, 100 ) == 0 && dm_grow( 0, 7 ) == 0 && dm_live() == 1 );
	CHECK( dm_grow( 0, 101 ) == 0 && dm_live() == 1 );
	dm_fail_at( 0 );
	CHECK( dm_grow( 0, 500 ) != 0 && dm_live() == 0 );
	CHECK( dm_alloc( 2, 9 ) == 0 && dm_alloc( 3, 4 ) == 0 );
	dm_swap( 2, 3 );
	dm_state( 2, s );
	CHECK( s[1] == 4 );
	dm_release( 2 );
	dm_release( 2 );
	dm_release( 3 );
	CHECK( dm_live() == 0 );

	int emptied[5], live[4], left = -1;

	for( int k = 0; k < 5; k++ ) {
		CHECK( dm_alloc_all( 8, emptied ) == 0 && dm_alloc_all_live() == 5 );
		const int before = dm_live() - 5;
		dm_fail_at( k );
		CHECK( dm_alloc_all( 8, emptied ) != 0 && dm_live() == before );

		for( int i = 0; i < 5; i++ ) {
			CHECK( emptied[i] == 1 );
		}
	}

	CHECK( dm_record( live ) == 5 && live[0] == 7 && live[1] == 14 && live[2] == 7 && live[3] == 0 );

	for( int k = 0; k < 7; k++ ) {
		CHECK( dm_record_fails( k, &left ) != 0 && left == 0 );
	}

	CHECK( dm_record_fails( 7, &left ) == 0 && left == 0 );
	dm_reset();
	CHECK( dm_live() == 0 && dm_null_releases() == 0 && dm_wrong_space() == 0 );
	std::printf( "device memory driver ok\n" );
	return 0;
}
#endif
