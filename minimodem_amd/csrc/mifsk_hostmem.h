// mifsk_hostmem.h -- who owns a device resource on the host side of libmifsk.so.
//
// Move-only owners, each with a destructor that gives back what it holds: DevMem<T> (hipMalloc),
// PinMem<T> (hipHostMalloc), StreamMem (hipMallocAsync, freed in the order of the stream it was made
// for), HipStream (a non-blocking stream, synchronised before it is destroyed) and HipEvent (an
// event without timing).  Every allocation, stream and event the library keeps is a member of one
// of these -- the context's cached tables and its chain, the host pipeline's work, a pipeline's
// lanes, a session, the legacy plan -- so dropping the struct that holds it frees it, once.  The one
// exception hands memory to the caller: mifsk_host_alloc / mifsk_host_free (mifsk_hostpipe.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstddef>
#include <utility>

namespace mifsk {

struct DeviceHeap {
    static hipError_t get( void **p, size_t bytes ) { return hipMalloc(p, bytes); }
    static void put( void *p ) { (void)hipFree(p); }
};

struct PinnedHeap {
    static hipError_t get( void **p, size_t bytes ) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void put( void *p ) { (void)hipHostFree(p); }
};

template <class T, class Heap>
struct OwnedMem {
    T		*p = nullptr;
    size_t	cap = 0;		// elements

    OwnedMem() = default;
    OwnedMem( OwnedMem &&o ) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    OwnedMem &operator=( OwnedMem &&o ) noexcept
    {
	if ( this != &o ) {
	    reset();
	    p = std::exchange(o.p, nullptr);
	    cap = std::exchange(o.cap, 0);
	}
	return *this;
    }
    ~OwnedMem() { reset(); }

    void reset() { if ( p ) Heap::put(p); p = nullptr; cap = 0; }
    T *release() { cap = 0; return std::exchange(p, nullptr); }	// the caller's to free from here on
    // room for n elements: what is there when it is enough, else a new block with 25 % head-room
    // (contents discarded); after a failure nothing is held
    int fit( size_t n )
    {
	if ( n <= cap )
	    return 0;
	reset();
	const size_t want = n + n / 4;
	if ( Heap::get((void **)&p, want * sizeof(T)) != hipSuccess ) {
	    p = nullptr;
	    return -ENOMEM;
	}
	cap = want;
	return 0;
    }
    // a new block of exactly n elements, min_bytes at least; `zero`: filled with zeros, and the fill
    // is done when this returns (before another stream writes into the block)
    int alloc( size_t n, size_t min_bytes = 0, bool zero = false )
    {
	reset();
	const size_t bytes = n * sizeof(T) > min_bytes ? n * sizeof(T) : min_bytes;
	if ( Heap::get((void **)&p, bytes) != hipSuccess ) {
	    p = nullptr;
	    return -ENOMEM;
	}
	cap = bytes / sizeof(T);
	return !zero || ( hipMemset(p, 0, bytes) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess ) ? 0 : -EIO;
    }
};

template <class T> using DevMem = OwnedMem<T, DeviceHeap>;
template <class T> using PinMem = OwnedMem<T, PinnedHeap>;

// per-call device scratch, allocated and freed in the order of stream `st`, 16 bytes at least
struct StreamMem {
    void	*p = nullptr;
    hipStream_t	st;

    explicit StreamMem( hipStream_t st_ ) : st(st_) {}
    StreamMem( StreamMem &&o ) noexcept : p(std::exchange(o.p, nullptr)), st(o.st) {}
    StreamMem &operator=( StreamMem &&o ) noexcept
    {
	if ( this != &o ) {
	    reset();
	    p = std::exchange(o.p, nullptr);
	    st = o.st;
	}
	return *this;
    }
    ~StreamMem() { reset(); }

    void reset() { if ( p ) (void)hipFreeAsync(p, st); p = nullptr; }
    void *release() { return std::exchange(p, nullptr); }
    int alloc( size_t bytes )
    {
	reset();
	if ( hipMallocAsync(&p, bytes > 16 ? bytes : 16, st) != hipSuccess ) {
	    p = nullptr;
	    return -ENOMEM;
	}
	return 0;
    }
};

// a stream or an event: make() keeps what is already held, so a creation that failed half-way
// through a set of them is finished by calling make() on the whole set again
struct StreamKind {
    using handle = hipStream_t;
    static hipError_t make( handle *h ) { return hipStreamCreateWithFlags(h, hipStreamNonBlocking); }
    static void drop( handle h ) { (void)hipStreamSynchronize(h); (void)hipStreamDestroy(h); }
};

struct EventKind {
    using handle = hipEvent_t;
    static hipError_t make( handle *h ) { return hipEventCreateWithFlags(h, hipEventDisableTiming); }
    static void drop( handle h ) { (void)hipEventDestroy(h); }
};

template <class Kind>
struct OwnedHandle {
    typename Kind::handle	h = nullptr;

    OwnedHandle() = default;
    OwnedHandle( OwnedHandle &&o ) noexcept : h(std::exchange(o.h, nullptr)) {}
    OwnedHandle &operator=( OwnedHandle &&o ) noexcept
    {
	if ( this != &o ) {
	    reset();
	    h = std::exchange(o.h, nullptr);
	}
	return *this;
    }
    ~OwnedHandle() { reset(); }

    void reset() { if ( h ) Kind::drop(h); h = nullptr; }
    int make()
    {
	if ( h )
	    return 0;
	if ( Kind::make(&h) != hipSuccess ) {
	    h = nullptr;
	    return -EIO;
	}
	return 0;
    }
    operator typename Kind::handle() const { return h; }
};

using HipStream = OwnedHandle<StreamKind>;	// non-blocking; synchronised, then destroyed
using HipEvent = OwnedHandle<EventKind>;	// timing disabled

} // namespace mifsk
