// Who owns device and pinned host memory: one move-only buffer type, and "all of these or none".  Host-only and free of HIP
// headers: the four primitives below are a link seam — pbr_hip.hip defines them over the HIP runtime,
// tests/device_memory_driver.cpp over malloc / free — so everything here is tested without a GPU.
#pragma once

#include <cstddef>
#include <initializer_list>

namespace ptmem {

// Defined by whoever links this header in.  The two alloc primitives return 0, or the hipError_t's value.  Hidden: a shared
// library's buffers call that library's primitives, whatever else the process has loaded.
#define PTMEM_SEAM __attribute__( ( visibility( "hidden" ) ) )
PTMEM_SEAM int deviceAlloc( void** p, size_t bytes );
PTMEM_SEAM void deviceFree( void* p );
PTMEM_SEAM int pinnedAlloc( void** p, size_t bytes );
PTMEM_SEAM void pinnedFree( void* p );
#undef PTMEM_SEAM

struct Device {
	static int alloc( void** p, size_t bytes ) { return deviceAlloc( p, bytes ); }
	static void free( void* p ) { deviceFree( p ); }
};

struct Pinned {
	static int alloc( void** p, size_t bytes ) { return pinnedAlloc( p, bytes ); }
	static void free( void* p ) { pinnedFree( p ); }
};

// count elements of T in Space, or nothing.  It converts to T*, so launches and copies read as they do with a raw pointer;
// a record of these is reset by assigning an empty record.  The release primitive is never called for a null pointer: a
// context that never reached the device goes without a call into the runtime.
template <class T, class Space = Device>
class Owned {
public:
	Owned() = default;
	Owned( const Owned& ) = delete;
	Owned& operator=( const Owned& ) = delete;
	Owned( Owned&& other ) noexcept { swap( other ); }
	~Owned() { reset(); }

	Owned& operator=( Owned&& other ) noexcept {
		if( this != &other ) {
			reset();
			swap( other );
		}

		return *this;
	}

	void reset() {
		if( p_ != nullptr ) {
			Space::free( p_ );
		}

		p_ = nullptr;
		count_ = 0;
	}

	// The old buffer goes FIRST (the largest one is a quarter of the device: it must never exist twice); at least 16 bytes are
	// asked for, so that an empty table still is a pointer a kernel may be handed.  On failure: empty.
	int alloc( size_t count ) {
		reset();
		void* p = nullptr;
		const size_t bytes = sizeof( T ) * count;
		const int err = Space::alloc( &p, bytes < 16 ? 16 : bytes );

		if( err == 0 ) {
			p_ = (T*) p;
			count_ = count;
		}

		return err;
	}

	// nothing when it holds that many already
	int grow( size_t count ) { return ( p_ != nullptr && count_ >= count ) ? 0 : alloc( count ); }

	void swap( Owned& other ) noexcept {
		T* const p = p_;
		const size_t count = count_;
		p_ = other.p_;
		count_ = other.count_;
		other.p_ = p;
		other.count_ = count;
	}

	T* get() const { return p_; }
	operator T*() const { return p_; }
	bool empty() const { return p_ == nullptr; }
	size_t count() const { return count_; }
	size_t bytes() const { return sizeof( T ) * count_; }   // of the elements: the 16-byte floor is not in it

private:
	T* p_ = nullptr;
	size_t count_ = 0;
};

// One entry of allocAll's list: a buffer of any element type and space, and the elements it is to hold.
struct Want {
	void* buffer;
	size_t count;
	int ( *alloc )( void*, size_t );
	void ( *reset )( void* );
};

template <class T, class Space>
Want want( Owned<T, Space>& buffer, size_t count ) {
	typedef Owned<T, Space> B;
	return { &buffer, count, []( void* b, size_t n ) { return ( (B*) b )->alloc( n ); }, []( void* b ) { ( (B*) b )->reset(); } };
}

// All of these or none, in the list's order: the first failure empties every buffer of the list and is returned.
inline int allocAll( std::initializer_list<Want> list ) {
	for( const Want& w : list ) {
		const int err = w.alloc( w.buffer, w.count );

		if( err != 0 ) {
			for( const Want& u : list ) {
				u.reset( u.buffer );
			}

			return err;
		}
	}

	return 0;
}

}  // namespace ptmem
