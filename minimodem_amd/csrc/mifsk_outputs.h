// mifsk_outputs.h -- the result arrays of mifsk_demod_io: the one place that lists them, for every
// host-side source that allocates, hands out, advances or copies back a set of them.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <utility>

#include "mifsk.h"
#include "mifsk_ctx.h"
#include "mifsk_hostmem.h"

namespace mifsk {

enum PerRow { kOne, kFramesCap, kEpisodesCap, kCounters };

struct OutArray {
    size_t	member;		// where its pointer is in mifsk_demod_io
    size_t	esz;		// bytes per element
    PerRow	per;		// elements per row
};

constexpr OutArray kOutArrays[] = {
    { offsetof(mifsk_demod_io, d_bytes), sizeof(uint8_t), kFramesCap },
    { offsetof(mifsk_demod_io, d_nbytes), sizeof(uint32_t), kOne },
    { offsetof(mifsk_demod_io, d_bits), sizeof(uint64_t), kFramesCap },
    { offsetof(mifsk_demod_io, d_frames), sizeof(mifsk_frame), kFramesCap },
    { offsetof(mifsk_demod_io, d_nframes), sizeof(uint32_t), kOne },
    { offsetof(mifsk_demod_io, d_episodes), sizeof(mifsk_episode), kEpisodesCap },
    { offsetof(mifsk_demod_io, d_nepisodes), sizeof(uint32_t), kOne },
    { offsetof(mifsk_demod_io, d_status), sizeof(uint32_t), kOne },
    { offsetof(mifsk_demod_io, d_counters), sizeof(uint64_t), kCounters },
    { offsetof(mifsk_demod_io, d_carrier_band), sizeof(int32_t), kOne },
};
constexpr size_t kNumOutArrays = sizeof(kOutArrays) / sizeof(kOutArrays[0]);
// a pipeline's output sets hold the arrays in front of these two (mifsk_pipeline.cpp)
constexpr size_t kNumPipelineArrays = kNumOutArrays - 2;
static_assert(kOutArrays[kNumPipelineArrays].member == offsetof(mifsk_demod_io, d_counters)
	      && kOutArrays[kNumPipelineArrays + 1].member == offsetof(mifsk_demod_io, d_carrier_band),
	      "the arrays a pipeline does not hand out are the table's last two");
// a new member of mifsk_demod_io stops the build here until the table has been looked at
static_assert(sizeof(mifsk_demod_io) == 3 * sizeof(void *) + 2 * sizeof(uint32_t)	// the five inputs
	      + kNumOutArrays * sizeof(void *) + 2 * sizeof(size_t)			// the arrays, frames_cap, episodes_cap
	      + 2 * sizeof(uint32_t),							// flags, reserved
	      "mifsk_demod_io has changed: is kOutArrays still the list of its result arrays?");

inline void *out_get( const mifsk_demod_io &io, const OutArray &a )
{
    void *p;
    std::memcpy(&p, (const char *)&io + a.member, sizeof(p));
    return p;
}

inline void out_set( mifsk_demod_io &io, const OutArray &a, void *p )
{
    std::memcpy((char *)&io + a.member, &p, sizeof(p));
}

inline size_t out_row_bytes( const mifsk_demod_io &io, const OutArray &a )
{
    const size_t per = a.per == kFramesCap ? io.frames_cap : a.per == kEpisodesCap ? io.episodes_cap
		     : a.per == kCounters ? (size_t)MIFSK_NCOUNTERS : 1;
    return per * a.esz;
}

// what a pipeline hands out of one of its sets: the set's arrays and the two capacities
inline void outputs_assign( mifsk_demod_io &dst, const mifsk_demod_io &src )
{
    for ( size_t i = 0; i < kNumPipelineArrays; i++ )
	out_set(dst, kOutArrays[i], out_get(src, kOutArrays[i]));
    dst.frames_cap = src.frames_cap;
    dst.episodes_cap = src.episodes_cap;
}

// The arrays a pipeline's MIFSK_WANT_* bits ask for, as the `want` of OutMirror::alloc, which only
// asks whether an array is there: the counts and the status always, any address standing for "yes".
inline mifsk_demod_io outputs_want( unsigned want, size_t frames_cap, size_t episodes_cap )
{
    void *const yes = const_cast<OutArray *>(kOutArrays);
    mifsk_demod_io io = {};
    io.frames_cap = frames_cap;
    io.d_nframes = io.d_nbytes = io.d_status = (uint32_t *)yes;
    io.d_bytes = ( want & MIFSK_WANT_BYTES ) ? (uint8_t *)yes : nullptr;
    io.d_bits = ( want & MIFSK_WANT_BITS ) ? (uint64_t *)yes : nullptr;
    io.d_frames = ( want & MIFSK_WANT_FRAMES ) ? (mifsk_frame *)yes : nullptr;
    if ( want & MIFSK_WANT_EPISODES ) {
	io.episodes_cap = episodes_cap ? episodes_cap : 1;
	io.d_episodes = (mifsk_episode *)yes;
	io.d_nepisodes = (uint32_t *)yes;
    }
    return io;
}

// every result array that is there, `rows` rows further on
inline void outputs_advance( mifsk_demod_io &io, size_t rows )
{
    for ( const OutArray &a : kOutArrays )
	if ( void *p = out_get(io, a) )
	    out_set(io, a, (char *)p + rows * out_row_bytes(io, a));
}

// The device mirror of a set of result arrays: `io` holds capacities and result pointers only
// (everything else 0), and the receive calls take it as it is; the memory behind is freed with
// the mirror.
struct OutMirror {
    mifsk_demod_io	io = {};
    DevMem<uint8_t>	mem[kNumOutArrays];

    OutMirror() = default;
    OutMirror( OutMirror &&o ) noexcept { *this = std::move(o); }
    OutMirror &operator=( OutMirror &&o ) noexcept	// (`io` points into `mem`, always: what is moved from is empty)
    {
	if ( this != &o ) {
	    for ( size_t i = 0; i < kNumOutArrays; i++ )
		mem[i] = std::move(o.mem[i]);
	    io = std::exchange(o.io, mifsk_demod_io{});
	}
	return *this;
    }
    void reset() { *this = OutMirror(); }
    // `want`'s capacities and a device array of `nrows` rows wherever `want` has an array.  `zero`:
    // the arrays are zero-filled, and the fill is done when this returns (before another stream
    // writes into them).
    int alloc( const mifsk_demod_io &want, size_t nrows, bool zero )
    {
	reset();
	io.frames_cap = want.frames_cap;
	io.episodes_cap = want.episodes_cap;
	for ( size_t i = 0; i < kNumOutArrays; i++ ) {
	    const OutArray &a = kOutArrays[i];
	    if ( !out_get(want, a) )
		continue;
	    const size_t bytes = std::max<size_t>(nrows * out_row_bytes(want, a), 16);
	    if ( const int rc = mem[i].alloc(bytes) )
		return rc;
	    out_set(io, a, mem[i].p);
	    if ( zero && hipMemset(mem[i].p, 0, bytes) != hipSuccess )
		return -EIO;
	}
	// (one wait for all the fills)
	return zero && hipStreamSynchronize(nullptr) != hipSuccess ? -EIO : 0;
    }
    // Rows [lo, hi) of the host arrays `ho` from the first hi - lo rows of the mirror, on `st`.  An
    // array that either side lacks is passed over.
    int copy_out( const mifsk_demod_io &ho, size_t lo, size_t hi, hipStream_t st, uint64_t *bytes_out ) const
    {
	for ( const OutArray &a : kOutArrays ) {
	    void *host = out_get(ho, a), *dev = out_get(io, a);
	    if ( !host || !dev )
		continue;
	    const size_t row = out_row_bytes(ho, a), nb = ( hi - lo ) * row;
	    HIP_OK(hipMemcpyAsync((char *)host + lo * row, dev, nb, hipMemcpyDeviceToHost, st));
	    *bytes_out += nb;
	}
	return 0;
    }
};

} // namespace mifsk
