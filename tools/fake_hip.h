// fake_hip.h -- the HIP runtime of the host-side checkers (hostmem_check.cpp, ctx_tables_check.cpp):
// device and page-locked memory are malloc(), streams and events are one-byte blocks of it, so that
// a leak, a double free and a use after a free are the address sanitizer's to report.  What is held
// is also counted here, and the N-th allocation, the N-th copy and the N-th stream or event can each
// be made to fail.  Included once, by the program's own source.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

struct Countdown { long n = 0, fail_at = 0; };		// fail_at: 1-based, 0 = never
static Countdown g_alloc, g_copy, g_make;
static long g_live = 0;					// allocations held
static long g_handles = 0, g_drops = 0;			// streams and events held; destroyed so far
static long g_syncs = 0, g_device_syncs = 0;
static const void *g_watch = nullptr;			// an allocation: how many stream synchronisations
static long g_watch_syncs = -1;				// had been seen when it was freed

static bool fails( Countdown &c ) { return ++c.n == c.fail_at; }

static hipError_t fake_alloc( void **p, size_t bytes )
{
    if ( fails(g_alloc) ) {
	*p = (void *)(uintptr_t)0xDEAD;			// (an owner must not keep what a failed call left)
	return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    std::memset(*p, 0xA5, bytes);
    g_live++;
    return hipSuccess;
}

static hipError_t fake_free( void *p )
{
    if ( p ) {
	if ( p == g_watch )
	    g_watch_syncs = g_syncs;
	g_live--;
	std::free(p);
    }
    return hipSuccess;
}

template <class H>
static hipError_t fake_make( H *h )
{
    if ( fails(g_make) ) {
	*h = (H)(uintptr_t)0xDEAD;
	return hipErrorOutOfMemory;
    }
    *h = (H)std::malloc(1);
    g_handles++;
    return hipSuccess;
}

template <class H>
static hipError_t fake_drop( H h )
{
    g_handles--;
    g_drops++;
    std::free((void *)h);
    return hipSuccess;
}

static hipError_t fake_copy( void *d, const void *s, size_t bytes )
{
    if ( fails(g_copy) )
	return hipErrorUnknown;
    std::memcpy(d, s, bytes);
    return hipSuccess;
}

hipError_t hipMalloc( void **p, size_t bytes ) { return fake_alloc(p, bytes); }
hipError_t hipFree( void *p ) { return fake_free(p); }
hipError_t hipHostMalloc( void **p, size_t bytes, unsigned ) { return fake_alloc(p, bytes); }
hipError_t hipHostFree( void *p ) { return fake_free(p); }
hipError_t hipMallocAsync( void **p, size_t bytes, hipStream_t ) { return fake_alloc(p, bytes); }
hipError_t hipFreeAsync( void *p, hipStream_t ) { return fake_free(p); }
hipError_t hipMemset( void *p, int v, size_t bytes ) { std::memset(p, v, bytes); return hipSuccess; }
hipError_t hipMemcpy( void *d, const void *s, size_t bytes, hipMemcpyKind ) { return fake_copy(d, s, bytes); }
hipError_t hipMemcpyAsync( void *d, const void *s, size_t bytes, hipMemcpyKind, hipStream_t ) { return fake_copy(d, s, bytes); }
hipError_t hipStreamCreateWithFlags( hipStream_t *s, unsigned ) { return fake_make(s); }
hipError_t hipStreamDestroy( hipStream_t s ) { return fake_drop(s); }
hipError_t hipEventCreateWithFlags( hipEvent_t *e, unsigned ) { return fake_make(e); }
hipError_t hipEventDestroy( hipEvent_t e ) { return fake_drop(e); }
hipError_t hipStreamSynchronize( hipStream_t ) { g_syncs++; return hipSuccess; }
hipError_t hipDeviceSynchronize() { g_device_syncs++; return hipSuccess; }
const char *hipGetErrorString( hipError_t ) { return "error"; }

// one gfx950 device
hipError_t hipGetDeviceCount( int *n ) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice( int ) { return hipSuccess; }
hipError_t hipGetDevice( int *d ) { *d = 0; return hipSuccess; }
hipError_t hipGetDeviceProperties( hipDeviceProp_t *prop, int )
{
    std::memset(prop, 0, sizeof(*prop));
    std::snprintf(prop->name, sizeof(prop->name), "fake");
    std::snprintf(prop->gcnArchName, sizeof(prop->gcnArchName), "gfx950:sramecc+:xnack-");
    prop->multiProcessorCount = 256;
    return hipSuccess;
}

static long g_checks = 0, g_failed = 0;

#define CHECK(cond)	do { g_checks++; if ( !( cond ) ) { g_failed++; \
	std::fprintf(stderr, "%s:%d: %s (alloc %ld, copy %ld, make %ld failing)\n", __FILE__, __LINE__, #cond, \
		     g_alloc.fail_at, g_copy.fail_at, g_make.fail_at); } } while (0)

// a scenario with event `fail_at` of one kind failing (0: none): returns how many of them it saw
template <class F>
static long run( Countdown &c, long fail_at, F scenario )
{
    c.n = 0;
    c.fail_at = fail_at;
    scenario();
    c.fail_at = 0;
    CHECK(g_live == 0 && g_handles == 0);		// everything a scenario made is gone behind it
    return c.n;
}

// a scenario once clean, then once for every event of that kind it sees, that one failing
template <class F>
static void every_failure( Countdown &c, F scenario )
{
    const long n = run(c, 0, scenario);
    CHECK(n > 0);
    for ( long k = 1; k <= n; k++ )
	run(c, k, scenario);
}
