// mifsk_rxloop.h -- what the two receive-loop kernels (master_loop in mifsk_kernels.hip,
// demod_wave_kernel in mifsk_wave.hip) set up in the same way: the length of a row, the cut of
// a chained launch, where a stream's results go, and a carrier episode's record.
// gfx950 only; included by .hip files only.
#pragma once

#include "mifsk_devlib.h"

namespace mifsk {

// The length of row s, never trusted beyond the row ...
__device__ __forceinline__ uint32_t row_nsamples( const mifsk_demod_io &io, uint32_t s )
{
    const uint32_t N = io.d_nsamples ? io.d_nsamples[s] : io.nsamples;
    return io.nstreams > 1 && (size_t)N > io.stream_stride ? (uint32_t)io.stream_stride : N;
}
// ... and what a chained launch of the resumable instantiation (ST, d_state given) sees of it:
// the first `limit` samples (0: all).  True when that cut N short.
// (N is cut in place: a second, uncut copy kept alive beside it moved the wavefront kernels'
// register allocation and cost NOAA SAME 0.25 %)
template <bool ST>
__device__ __forceinline__ bool chain_cut( const mifsk_stream_state *d_state, uint32_t limit, uint32_t &N )
{
    if constexpr ( ST ) {
	if ( d_state && limit != 0u && limit < N ) {
	    N = limit;
	    return true;
	}
    }
    return false;
}

// Where stream s writes its results.  Made once: the serial loop is latency-bound, and a scalar
// kept in (or spilled to a VGPR lane from) a register costs a cycle where a reload from the
// kernarg segment costs a scalar-cache round trip per block of frames (measured with the
// pointers re-made at every use: configs[1] 0.45 -> 0.52 ms, 12000 baud 1.29 -> 1.79 ms).
// The capacities are clamped to 32 bits: every index compared with them is a 32-bit count of
// frames of one row, which holds fewer than 2^32 - 1 samples, so no comparison changes.
struct StreamOut {
    uint8_t		*bytes;
    uint64_t		*bits;
    mifsk_frame		*frames;
    mifsk_episode	*eps;
    uint32_t		fcap, ecap;

    static __device__ __forceinline__ StreamOut make( const mifsk_demod_io &io, uint32_t s )
    {
	StreamOut o;
	o.fcap = (uint32_t)( io.frames_cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : io.frames_cap );
	o.ecap = (uint32_t)( io.episodes_cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : io.episodes_cap );
	o.bytes = io.d_bytes ? io.d_bytes + (size_t)s * io.frames_cap : nullptr;
	o.bits = io.d_bits ? io.d_bits + (size_t)s * io.frames_cap : nullptr;
	o.frames = io.d_frames ? io.d_frames + (size_t)s * io.frames_cap : nullptr;
	o.eps = io.d_episodes ? io.d_episodes + (size_t)s * io.episodes_cap : nullptr;
	return o;
    }
};

// One carrier episode (minimodem.c:1292-1321 at carrier loss: end_reason 1; :1469-1474 at the
// end of the stream: 2), stored at index n_out_eps by the lane that is `writer`, if the caller
// wants episodes and has room.  The kernel counts it either way.  The loop state is taken by
// value: the kernels keep it in plain local scalars.
__device__ __forceinline__ void store_episode( const StreamOut &o, bool writer, uint32_t n_out_eps,
	uint64_t carrier_nsamples, uint32_t ep_first, uint32_t nframes_decoded, float confidence_total,
	float amplitude_total, uint32_t end_reason, uint32_t b_mark )
{
    if ( writer && o.eps && n_out_eps < o.ecap ) {
	mifsk_episode e;
	e.carrier_nsamples = carrier_nsamples;
	e.first_frame = ep_first;
	e.nframes = nframes_decoded;
	e.confidence_total = confidence_total;
	e.amplitude_total = amplitude_total;
	e.end_reason = end_reason;
	e.b_mark = b_mark;
	o.eps[n_out_eps] = e;
    }
}

} // namespace mifsk
