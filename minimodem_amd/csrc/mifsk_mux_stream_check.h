// mifsk_mux_stream_check.h -- the host logic of a multiplexer stream (include/mifsk/mux_stream.h,
// mifsk_mux_stream.hip) that needs no device: the samples a later output still reads, a stream's record
// (its tails have stream_tail_room of H, mifsk_stream_check.h, which holds what the two streams
// share), and what a feed refuses of its arguments.  It calls no HIP: tools/mux_stream_check.cpp runs
// it on a CPU under the sanitizers (tests/test_mux_stream_args.py).
#pragma once

#include <cerrno>
#include <cstdint>

#include "mifsk.h"
#include "mifsk/mux_stream.h"
#include "mifsk_batch.h"
#include "mifsk_stream_check.h"

namespace mifsk {

// H: output n = m L + phi reads the samples m, m - 1, ..., m - ceil(T / L) + 1, so the first outputs of
// a piece read the last ceil(T / L) - 1 samples of the piece before.  0 without an interpolation.
inline uint32_t mux_stream_drain( uint32_t T, uint32_t L )
{
    return L != 0u && T != 0u ? ( T - 1u ) / L : 0u;		// ceil(T / L) - 1 = floor((T - 1) / L)
}

// What a stream keeps between feeds: the samples it has taken, and the absolute index in front of
// which samples do not exist (0, or where a seek joined).  first <= seen always.
struct MuxStreamRecord {
    uint64_t	seen, first;
};

// a seek's record: nothing in front of n0 is ever read
inline MuxStreamRecord mux_stream_record_at( uint64_t n0 ) { return MuxStreamRecord{n0, n0}; }

// seeks go this far: seen * L stays below 2^62 for any L <= 65535
constexpr uint64_t kMuxStreamMaxSeen = 1ull << 46;

// tail samples that exist: those of the last H at or behind `first`
__host__ __device__ inline uint32_t mux_stream_back( uint32_t H, const MuxStreamRecord &r )
{
    const uint64_t have = r.seen - r.first;
    return have < H ? (uint32_t)have : H;
}

// what a feed has to know of its object
struct MuxStreamShape {
    bool	cx, s16;	// the plan's kind: the output's
    bool	iq;		// input rows are (I, Q) pairs
    uint32_t	L, K;		// ... its interpolation and channels
    int		nstreams;
};

// kmax * L outputs fit into `room` elements (64 bits: kmax < 2^32, L < 2^16)
inline bool mux_stream_fits( uint64_t kmax, uint32_t L, uint64_t room ) { return kmax * (uint64_t)L <= room; }

// What mifsk_mux_stream_feed refuses behind the NULL object and io, in the header's order: everything
// the batch entry of the object's input kind refuses of the io, a number of streams that is not the
// object's, then an out_stride and a nout_cap below kmax * L: a feed delivers exactly k_s L outputs,
// and dropping one would break the continuation.
inline int mux_stream_feed_check( const MuxStreamShape &sh, const mifsk_mux_io *io )
{
    if ( int rc = rows_io_check(sh.K, io, io->d_out, sh.iq ? 2u : 4u, rows_vec(sh.cx, sh.s16), 0xFFFFFFF8ull) )
	return rc;
    if ( io->nstreams != sh.nstreams )
	return -EINVAL;
    const uint64_t kmax = stream_kmax(io);
    if ( !mux_stream_fits(kmax, sh.L, io->out_stride) )
	return -EINVAL;
    if ( !mux_stream_fits(kmax, sh.L, io->nout_cap) )
	return -EINVAL;
    return 0;
}

} // namespace mifsk
